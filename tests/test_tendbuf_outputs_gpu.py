"""The prognostic step and the in-place checks on packed tendency buffers, on the device:
cloudsc_gpu_run_tendbuf_outputs(PROGNOSTIC) against cloudsc_gpu_run on a second set holding the same inputs
in separate arrays -- on the device with cloudsc_fields_compare_tendbuf (planes n against 0, the ten
diagnostic members NULL in both) and again on the host, on raw bits, with the sentinels of unbound planes,
padding lanes and non-NULL diagnostic members; cloudsc_fields_expand_tendbuf and
cloudsc_fields_validate_tendbuf against the parent path (expand / validate on separate arrays around
cloudsc_fields_convert_tendbuf); and the CLI's --fields tendbuf-inplace and --outputs prognostic."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import cloudsc_amd as ca
import host_harness as hh
import tendbuf_cases as tb
from gpu_harness import CASES as SHAPE_CASES, DIAG, DeviceSide, KEPT, NAMES, PRECISIONS, ProgPair, VARIANTS
from gpu_harness import oracle_columns, validation_table, without_diag
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PROG, ALL = ca.OUTPUTS_PROGNOSTIC, ca.OUTPUTS_ALL
# (planes, order, the ten diagnostic members of the packed set): 8 in the reference order with them NULL,
# 11 permuted (three unbound planes) with them pointing at arrays that must keep every byte
SETTINGS = [(8, "reference", "null"), (11, "permuted", "kept")]
CASES = SHAPE_CASES + [(1, 1, "kcache"), (1, 1, "kseg")]


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("ngptot,nproma,variant", CASES)
def test_run_tendbuf_prognostic_bitwise(lib, hip, ds, oracle_mod, ngptot, nproma, variant, precision):
    prec = PRECISIONS[precision]
    for tend_planes, order, diag in SETTINGS:
        pr = ProgPair(lib, hip, ds, ngptot, nproma, prec, tend_planes, order)
        try:
            if nproma == 32:
                ca.narrow_pack(1)
            geo = ca.launch_geometry(prec, VARIANTS[variant], ngptot, nproma, ds.klev)
            assert geo["pack"] == (64 // nproma if nproma <= 32 else 1)
            pr.fill()
            pr.run_both(VARIANTS[variant], which=("plain",))
            pr.run_form(VARIANTS[variant], PROG, diag)
            assert pr.device_mismatches_inplace() == {}
            assert pr.host_check_form() == []
            if prec == ca.FP64:
                got, exp = pr.kept_columns(), oracle_columns(oracle_mod, ds, "ds", ngptot, nproma)
                assert [k for k in KEPT if not np.array_equal(tb.bits(got[k]), tb.bits(exp[k]))] == []
        finally:
            pr.close()


def test_run_tendbuf_prognostic_aerosols(lib, hip, ds):
    import make_fixtures as mf
    s = mf.with_aerosols(ds)
    for variant, nproma in ((ca.VARIANT_KSEG, 64), (ca.VARIANT_KCACHE, 16)):
        pr = ProgPair(lib, hip, s, 100, nproma, ca.FP64, 11, "permuted")
        try:
            assert pr.aer
            pr.fill()
            pr.run_both(variant, which=("plain",))
            pr.run_form(variant)
            assert pr.device_mismatches_inplace() == {}
            assert pr.host_check_form() == []
        finally:
            pr.close()


def test_run_tendbuf_prognostic_non_default_stream(lib, hip, ds):
    pr = ProgPair(lib, hip, ds, 200, 128, ca.MIXED, 11, "permuted")
    st = C.c_void_p()
    try:
        assert hip.hipStreamCreateWithFlags(C.byref(st), C.c_uint(1)) == 0      # hipStreamNonBlocking
        pr.fill()
        hip.hipDeviceSynchronize()
        pr.run_both(ca.VARIANT_KSEG, stream=st, which=("plain",))
        pr.run_form(ca.VARIANT_KSEG, PROG, "kept", stream=st)
        assert pr.device_mismatches_inplace(stream=st) == {}
        assert hip.hipStreamSynchronize(st) == 0
        assert pr.host_check_form() == []
    finally:
        if st.value:
            hip.hipStreamDestroy(st)
        pr.close()


def test_run_tendbuf_prognostic_few_workgroups_many_handoffs(lib, hip, ds):
    pr = ProgPair(lib, hip, ds, 300, 64, ca.FP64, 8, "reference")
    try:
        pr.fill()
        pr.run_both(ca.VARIANT_KSEG, which=("plain",))
        ca.kseg_schedule(3, 3)
        pr.run_form(ca.VARIANT_KSEG)
        assert pr.device_mismatches_inplace() == {}
        assert pr.host_check_form() == []
    finally:
        pr.close()


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_all_prognostic_all_on_one_workspace(lib, hip, ds, precision):
    """One KSEG workspace serves the forms in any order; OUTPUTS_ALL is cloudsc_gpu_run_tendbuf."""
    pr = ProgPair(lib, hip, ds, 300, 64, PRECISIONS[precision], 11, "permuted")
    try:
        pr.fill()
        pr.run_both(ca.VARIANT_KSEG, which=("plain",))
        for outputs in (ALL, PROG, ALL):
            pr.fill(("packed",))
            pr.run_form(ca.VARIANT_KSEG, outputs, "kept")
            names = KEPT if outputs == PROG else tuple(NAMES)
            assert pr.device_mismatches_inplace(names) == {}, outputs
            assert pr.host_check_form(outputs) == [], outputs
    finally:
        pr.close()


# ---------------------------------------------------------------------------
# fill and validate in place
# ---------------------------------------------------------------------------
def levels_dataset(ds, scenarios, klev):
    import form_state_cases as fs
    if klev == 137:
        return ds
    return fs.dataset({3: "klev3", 274: "klev274"}[klev], ds, scenarios)


@pytest.mark.parametrize("klev", [137, 3, 274])
@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_expand_tendbuf_against_expand_and_pack(lib, hip, ds, scenarios, klev, precision):
    """cloudsc_fields_expand_tendbuf against the parent path (cloudsc_fields_expand into separate arrays, then
    cloudsc_fields_convert_tendbuf), compared in place on the device (the two sides in blocks of 64 and 16, 11
    permuted planes against 8) and on the host as whole buffers: unbound planes and padding lanes keep their
    sentinels."""
    s, prec, n = levels_dataset(ds, scenarios, klev), PRECISIONS[precision], 300
    inputs = [k for k in ca.INPUT_FIELDS if k in ca.ALL_FIELDS and not k.startswith(("pre_ice", "picrit", "pnice"))]
    keep = []
    tmpl = ca.make_template(s, keep)
    for (np_a, planes_a, order_a), (np_b, prec_b) in (((64, 11, "permuted"), (16, prec)),
                                                     ((16, 8, "reference"), (64, prec))):
        a = ProgPair(lib, hip, s, n, np_a, prec, planes_a, order_a)
        b = ProgPair(lib, hip, s, n, np_b, prec_b, 8, "reference")
        try:
            for pr in (a, b):     # sentinels everywhere in the two buffers
                sent = tb.empty_buffer(pr.nb, pr.tend_planes, s.klev, pr.nproma, pr.buf_tmp.dtype, tb.SENTINEL_TMP)
                assert hip.hipMemcpy(pr.packed.buffer_tmp, sent.ctypes.data, sent.nbytes, 1) == 0
                assert hip.hipMemcpy(pr.packed.buffer_loc, pr.buf_loc.ctypes.data, pr.buf_loc.nbytes, 1) == 0
            # a: in place.  b: the parent path
            ca.expand_fields_tendbuf(ca.fields_subset(a.packed.f, inputs), tmpl, prec, n, np_a, planes_a)
            b.packed.expand(s)
            ca.convert_fields_tendbuf(ca.fields_subset(b.packed.separate, tb.TMP), ca.fields_subset(b.packed.f, tb.TMP),
                                      n, s.klev, prec_b, np_b, 0, prec_b, np_b, 8)
            d = ca.compare_fields_tendbuf(ca.fields_subset(a.packed.f, inputs), ca.fields_subset(b.packed.f, inputs), n,
                                          s.klev, prec, np_a, planes_a, prec_b, np_b, 8)
            assert sorted(d) == sorted(inputs) and all(v["compared"] > 0 for v in d.values())
            assert {k: v["mismatches"] for k, v in d.items() if v["mismatches"]} == {}
            # on the host: BUFFER_TMP of a, whole
            hip.hipDeviceSynchronize()
            got = np.empty_like(a.buf_tmp)
            assert hip.hipMemcpy(got.ctypes.data, a.packed.buffer_tmp, got.nbytes, 2) == 0
            assert np.array_equal(tb.bits(got), tb.bits(a.buf_tmp))        # Pair's NumPy packing of the same values
            loc = np.empty_like(a.buf_loc)
            assert hip.hipMemcpy(loc.ctypes.data, a.packed.buffer_loc, loc.nbytes, 2) == 0
            assert tb.is_sentinel(loc, np.ones(loc.shape, bool), tb.SENTINEL_LOC)      # outputs are not filled
        finally:
            a.close()
            b.close()


def tall_pair(ngptot, anp, bnp, klev, ap, bp, names):
    """fields_compare_cases.make_pair where its encoder reaches (fewer than 1024 rows); beyond that (the species
    members at KLEV 274: 1370 rows) the same construction with (row, column) in 11 + 9 bits: values exact in
    float, different NaN words in the padding lanes, b changed at the positions make_pair plants."""
    import fields_compare_cases as cc
    import fields_convert_cases as fc
    if max(fc.rows_of(n, klev) for n in names) < 1024:
        return cc.make_pair(ngptot, anp, bnp, klev, ap, bp, names=names)
    assert ngptot <= 512 and max(fc.rows_of(n, klev) for n in names) < 2048
    rng = np.random.default_rng(cc.SEED)
    acols = {n: ((np.arange(fc.rows_of(n, klev), dtype=np.int64)[:, None] << 9) +
                 np.arange(ngptot, dtype=np.int64)[None, :] + (names.index(n) << 20)).astype(np.float64) for n in names}
    bcols = {n: v.copy() for n, v in acols.items()}
    pos = cc.planted(names, klev, ngptot, rng)
    for n, row, g in pos:
        bcols[n][row, g] = bcols[n][row, g] + 1 if n == "ktype" else (2 * int(rng.integers(1 << 19)) + 1) / 64.0
    a = cc.fill_set(fc.HostSet(ngptot, anp, klev, ap, names=names), acols, cc.NAN_A)
    b = cc.fill_set(fc.HostSet(ngptot, bnp, klev, bp, names=names), bcols, cc.NAN_B)
    return a, b, pos


@pytest.mark.parametrize("klev", [3, 137, 274])
def test_device_compare_tendbuf_against_host_twin(lib, hip, klev):
    """cloudsc_fields_compare_tendbuf against cloudsc_cpu_fields_compare_tendbuf (itself pinned to NumPy in
    tests/test_tendbuf_outputs_cpu.py): 300 columns (a tile boundary crossed), blocks of 64 against 16, fp64
    against float, 11 permuted planes against 0 and against 8, planted differences, grids of 1 and 3
    workgroups: every field that must not depend on the grouping is equal."""
    import fields_compare_cases as cc
    names = list(tb.TMP + tb.LOC) + ["pt", "pfplsl", "ktype", "prainfrac_toprfz"]
    for bpl in (0, 8):
        ha, hb, pos = tall_pair(300, 64, 16, klev, ca.FP64, ca.MIXED, names)
        a, b = hh.PackedSide(ha, 11), hh.PackedSide(hb, bpl, "reference")
        tb.bits(a.bufs[1])[0, sorted(set(range(11)) - {a.lay[n] + i for n in tb.LOC for i in range(tb.nplanes(n))})[0],
                           0, 0] ^= 1                                        # an unbound plane: never read
        want = hh.cpu_compare(a, b)
        assert sum(d.mismatches for d in want) >= len(set(pos))
        da, db = DeviceSide(hip, a), DeviceSide(hip, b)
        try:
            for grid in (1, 3, 0):
                ca.compare_grid(grid)
                got = cc.new_diffs()
                ca.check(lib.cloudsc_fields_compare_tendbuf(0, None, 300, klev, ca.FP64, 64, 11, C.byref(da.f),
                                                            ca.MIXED, 16, bpl, C.byref(db.f), got))
                for m in range(len(got)):
                    assert cc.exact_fields(got[m]) == cc.exact_fields(want[m]), (m, grid, bpl)
                    assert (got[m].stats.errsum, got[m].stats.refsum) == (want[m].stats.errsum, want[m].stats.refsum)
        finally:
            da.close()
            db.close()


def stats_tuple(s):
    return (s.minval, s.maxval, s.maxerr, s.errsum, s.refsum, s.errsum_lo, s.refsum_lo)


def same_stats(got, want, count):
    """min, max and max error exactly; each sum as tests/test_fields_compare_gpu.py holds the device against the
    host twin: the high parts equal, and hi + lo within count * 2^-100 of the other's (the bound derived in
    tests/fields_compare_cases.py for `count` elements)."""
    if got[:3] != want[:3]:
        return False
    for hi, lo, whi, wlo in ((got[3], got[5], want[3], want[5]), (got[4], got[6], want[4], want[6])):
        a, b = Fraction(hi) + Fraction(lo), Fraction(whi) + Fraction(wlo)
        if hi != whi or abs(a - b) > count * Fraction(1, 2 ** 100) * b:
            return False
    return True


SKIPPED = (np.finfo(np.float64).max, -np.finfo(np.float64).max, 0.0, 0.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
@pytest.mark.parametrize("nproma,tend_planes,order", [(64, 11, "permuted"), (16, 8, "reference")])
def test_validate_tendbuf_against_validate(lib, hip, ds, precision, nproma, tend_planes, order):
    """stats[] of the in-place validation of BUFFER_LOC = cloudsc_fields_validate on the unpacked arrays: min,
    max, max error exactly; the sums within the double-double bound (their high parts equal: the bound,
    n * 2^-100 relative, is far below half an ulp of the high part); on grids of 1 and 3 workgroups."""
    prec, n = PRECISIONS[precision], 300
    names = [k for _, k in ca.VALIDATED]
    pr = ProgPair(lib, hip, ds, n, nproma, prec, tend_planes, order)
    try:
        pr.fill()
        pr.run_form(ca.VARIANT_KSEG, ALL, "kept")
        # the parent path: unpack, validate the separate arrays
        ca.convert_fields_tendbuf(ca.fields_subset(pr.packed.f, tb.LOC), ca.fields_subset(pr.packed.separate, tb.LOC),
                                  n, ds.klev, prec, nproma, tend_planes, prec, nproma, 0)
        want = pr.packed.validate(ds)
        keep = []
        ref = ca.make_reference(ds, keep)
        ref_prog = ca.make_reference(ds, keep)
        for i, k in enumerate(names):
            if k in DIAG:
                ref_prog.field[i] = None
        for grid in (1, 3, 0):
            ca.compare_grid(grid)
            got = [stats_tuple(s) for s in ca.validate_fields_tendbuf(pr.packed.f, ref, prec, n, nproma, ds.klev,
                                                                      tend_planes, ALL)]
            prog = [stats_tuple(s) for s in ca.validate_fields_tendbuf(without_diag(pr.packed.f), ref_prog, prec, n,
                                                                       nproma, ds.klev, tend_planes, PROG)]
            sep = [stats_tuple(s) for s in ca.validate_fields_tendbuf(without_diag(pr.packed.separate), ref_prog, prec,
                                                                      n, nproma, ds.klev, 0, PROG)]
            for i, k in enumerate(names):
                count = int(np.prod(ca.field_shape(ca.ALL_FIELDS[k], ds.klev, n)))
                assert same_stats(got[i], want[i], count), (k, grid, got[i], want[i])
                if k in DIAG:
                    assert prog[i] == SKIPPED and sep[i] == SKIPPED, (k, grid)
                else:
                    assert same_stats(prog[i], want[i], count), (k, grid, prog[i], want[i])
                    assert same_stats(sep[i], want[i], count), (k, grid, sep[i], want[i])
    finally:
        pr.close()


# ---------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------
EXE = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")


def cli(*args):
    r = subprocess.run([EXE, "1", "300", "64"] + list(args), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_tendbuf_inplace_prints_callers_tables():
    caller = validation_table(cli("--fields", "caller"))
    inplace = validation_table(cli("--fields", "tendbuf-inplace"))
    assert len(inplace) == 23 and inplace == caller
    planes = validation_table(cli("--fields", "tendbuf-inplace", "--tend-planes", "11"))
    assert planes == caller


@pytest.mark.parametrize("common", [[], ["--variant", "kcache", "--precision", "mixed"]], ids=["default", "kcache_mixed"])
def test_cli_outputs_prognostic(common):
    full = validation_table(cli("--fields", "caller", *common))
    assert len(full) == 23
    kept_rows = [ln for ln in full[1:-1] if ln.split()[0].lower() not in [d.lower() for d in DIAG]]
    assert len(kept_rows) == 11
    for fields in ("caller", "tendbuf", "tendbuf-inplace"):
        out = cli("--fields", fields, "--outputs", "prognostic", *common)
        table = validation_table(out)
        assert table[0] == full[0]
        assert table[1:-1] == kept_rows, fields
        assert table[-1].split("(")[0] == full[-1].split("(")[0]            # VALIDATION: PASSED / reported only
        # the JUBE patterns of tests/test_stdout_contract.py: the timing rows, and each kept field's five values
        hh.check_timing(out, 1, 300, 64, 5)
        for (f, col), pat in hh.result_patterns().items():
            flags = re.IGNORECASE if f.startswith("tendency") else 0
            found = re.findall(hh.jube(pat), out, flags)
            assert len(found) == (0 if f.lower() in DIAG else 1), (fields, f, col, found)
        assert cli("--fields", fields, "--outputs", "all", *common).splitlines()[-23:] == full
