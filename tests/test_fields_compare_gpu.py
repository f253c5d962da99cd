"""Field set comparison, validation and expansion on the device (cloudsc_fields_compare / _validate /
_expand): the cases of tests/test_fields_compare_cpu.py against the host twin (itself held to the
restatement there), expansion against ca.expand, validation against the state API and an exact host restatement, the physics kernels
held against each other through the comparison, and the CLI's --fields caller."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import cloudsc_amd as ca
import fields_compare_cases as cc
import fields_convert_cases as fc
from gpu_harness import lib, hip, run_on  # noqa: F401  (lib, hip: fixtures)

pytestmark = pytest.mark.gpu

INPUTS = list(ca.INPUT_FIELDS) + list(ca.INOUT_FIELDS)
OUTPUTS = cc.OUTPUTS
PRECISIONS = [ca.FP64, ca.FP32, ca.MIXED]
PRECISION_IDS = ["fp64", "fp32", "mixed"]


def host_compare(lib, a, b, names=None):
    d = cc.new_diffs()
    ca.check(lib.cloudsc_cpu_fields_compare(2, a.ngptot, a.klev, a.precision, a.nproma, C.byref(a.fields(names)),
                                            b.precision, b.nproma, C.byref(b.fields(names)), d))
    return d


def on_device(hs):
    """A HostSet uploaded as it is (padding lanes included) into a DeviceFields."""
    d = ca.DeviceFields(hs.ngptot, hs.nproma, hs.klev, hs.precision, place=False, aerosols=True)
    d.upload(hs.arrays)
    return d


def device_compare(lib, da, db, names, stream=None):
    d = cc.new_diffs()
    ca.check(lib.cloudsc_fields_compare(0, stream, da.ngptot, da.klev, da.precision, da.nproma,
                                        C.byref(ca.fields_subset(da.f, names)), db.precision, db.nproma,
                                        C.byref(ca.fields_subset(db.f, names)), d))
    return d


def assert_sums_close(x_hi, x_lo, y_hi, y_lo, n, what):
    """hi equal, and hi + lo within n * 2^-100 of the other's (fields_compare_cases: the derived bound)."""
    assert x_hi == y_hi, (what, x_hi, y_hi)
    ref = cc.dd_value(y_hi, y_lo)
    assert abs(cc.dd_value(x_hi, x_lo) - ref) <= n * Fraction(1, 2 ** 100) * ref, (what, x_hi, x_lo, y_hi, y_lo)


def assert_same_as_host(dev, host):
    for m, n in enumerate(fc.MEMBERS):
        assert cc.exact_fields(dev[m]) == cc.exact_fields(host[m]), (n, cc.exact_fields(dev[m]), cc.exact_fields(host[m]))
        d, h, cnt = dev[m].stats, host[m].stats, max(host[m].compared, 1)
        assert_sums_close(d.errsum, d.errsum_lo, h.errsum, h.errsum_lo, cnt, n + " errsum")
        assert_sums_close(d.refsum, d.refsum_lo, h.refsum, h.refsum_lo, cnt, n + " refsum")


# ---------------------------------------------------------------------------
# the device against the host twin
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ap,bp", cc.STORAGE, ids=cc.STORAGE_IDS)
@pytest.mark.parametrize("ngptot,anp,bnp", cc.SHAPES)
def test_device_matches_host_twin(lib, ngptot, anp, bnp, ap, bp):
    a, b, pos = cc.make_pair(ngptot, anp, bnp, cc.KLEV, ap, bp)
    host = host_compare(lib, a, b)
    assert sum(host[m].mismatches for m in range(len(fc.MEMBERS))) == len(set(pos))
    da, db = on_device(a), on_device(b)
    try:
        assert_same_as_host(device_compare(lib, da, db, a.names), host)
    finally:
        da.close()
        db.close()


@pytest.fixture(scope="module")
def tall(lib):
    """(1000, 64, 24) at KLEV 137, fp64 against float storage, the outputs: host sets, host twin, device sets"""
    a, b, _ = cc.make_pair(1000, 64, 24, cc.TALL_KLEV, ca.FP64, ca.MIXED, names=OUTPUTS)
    host = host_compare(lib, a, b)
    da = ca.DeviceFields(1000, 64, cc.TALL_KLEV, ca.FP64, place=False)
    db = ca.DeviceFields(1000, 24, cc.TALL_KLEV, ca.MIXED, place=False)
    da.upload(a.arrays)
    db.upload(b.arrays)
    yield a, b, host, da, db
    da.close()
    db.close()


@pytest.mark.parametrize("ap,bp", cc.STORAGE, ids=cc.STORAGE_IDS)
@pytest.mark.parametrize("ngptot,anp,bnp", cc.TALL_SHAPES)
def test_device_klev_137(lib, ngptot, anp, bnp, ap, bp):
    a, b, _ = cc.make_pair(ngptot, anp, bnp, cc.TALL_KLEV, ap, bp, names=OUTPUTS)
    host = host_compare(lib, a, b)
    da = ca.DeviceFields(ngptot, anp, cc.TALL_KLEV, ap, place=False)
    db = ca.DeviceFields(ngptot, bnp, cc.TALL_KLEV, bp, place=False)
    try:
        da.upload(a.arrays)
        db.upload(b.arrays)
        assert_same_as_host(device_compare(lib, da, db, OUTPUTS), host)
    finally:
        da.close()
        db.close()


def test_grid_independence(lib, tall):
    """1 workgroup, 3 workgroups (fewer than members: every workgroup walks many items of every member) and
    the default grid: the same exact fields, the same rounded sums."""
    a, b, host, da, db = tall
    runs = []
    try:
        for grid in (1, 3, 0):
            ca.compare_grid(grid)
            runs.append(device_compare(lib, da, db, OUTPUTS))
    finally:
        ca.compare_grid(0)
    for r in runs:
        assert_same_as_host(r, host)
    for m in range(len(fc.MEMBERS)):
        assert len({(r[m].stats.errsum, r[m].stats.refsum) for r in runs}) == 1


def test_non_default_stream_and_python_form(lib, hip, tall):
    a, b, host, da, db = tall
    st = C.c_void_p()
    try:
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipStreamCreateWithFlags(C.byref(st), C.c_uint(1)) == 0      # hipStreamNonBlocking
        assert_same_as_host(device_compare(lib, da, db, OUTPUTS, stream=st), host)
        got = da.compare(db, names=OUTPUTS, stream=st)
    finally:
        if st.value:
            hip.hipStreamDestroy(st)
    assert sorted(got) == sorted(OUTPUTS)
    for n in OUTPUTS:
        h = host[fc.MEMBERS.index(n)]
        assert (got[n]["compared"], got[n]["mismatches"]) == (h.compared, h.mismatches)
        assert got[n]["first"] == ((h.first_column, h.first_row) if h.mismatches else None)
        assert got[n]["stats"][:5] == (h.stats.minval, h.stats.maxval, h.stats.maxerr, h.stats.errsum, h.stats.refsum)


CHILD = r"""
import ctypes as C, sys
import cloudsc_amd as ca, fields_compare_cases as cc, fields_convert_cases as fc
lib = ca.gpu_lib()
a, b, pos = cc.make_pair(150, 24, 64, cc.KLEV, ca.FP64, ca.MIXED)
da = ca.DeviceFields(150, 24, cc.KLEV, ca.FP64, place=False, aerosols=True)
db = ca.DeviceFields(150, 64, cc.KLEV, ca.MIXED, place=False, aerosols=True)
da.upload(a.arrays); db.upload(b.arrays)
got = da.compare(db)            # no cloudsc_gpu_init in this process
ca.check(lib.cloudsc_fields_compare_release(0))
again = da.compare(db)          # the workspace comes back after a release
assert {n: g["mismatches"] for n, g in got.items()} == {n: g["mismatches"] for n, g in again.items()}
print("MISMATCHES", sum(g["mismatches"] for g in got.values()), len(set(pos)))
da.close(); db.close()
"""


def test_before_any_gpu_init(lib):
    """A fresh process that never calls cloudsc_gpu_init: the comparison works, also after a release."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(ca.__file__), os.path.dirname(cc.__file__)]))
    out = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("MISMATCHES")][0].split()
    assert line[1] == line[2] and int(line[1]) > 0


# ---------------------------------------------------------------------------
# expansion
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS, ids=PRECISION_IDS)
@pytest.mark.parametrize("col_offset", [0, 37])
@pytest.mark.parametrize("ngptot,nproma", [(300, 64), (150, 24)])
def test_expand(lib, ds, ngptot, nproma, col_offset, precision):
    df = ca.DeviceFields(ngptot, nproma, ds.klev, precision, place=False)
    try:
        held = [n for n in ca.ALL_FIELDS if getattr(df.f, n)]
        sentinel = fc.HostSet(ngptot, nproma, ds.klev, precision, names=held)
        df.upload(sentinel.arrays)
        df.expand(ds, col_offset)
        got = {n: df.download_raw(n) for n in held}
    finally:
        df.close()
    nb = ca.nblocks_of(ngptot, nproma)
    active = (np.arange(nb * nproma) < ngptot).reshape(nb, 1, nproma)
    for n in held:
        g = got[n].reshape(sentinel.arrays[n].shape)
        want = sentinel.arrays[n].copy()                       # outputs and padding lanes: still the sentinel
        if n in INPUTS:
            dt = fc.dtype_of(n, precision)
            e = ca.expand(ds.inputs[n], ca.ALL_FIELDS[n], ngptot, nproma, col_offset, dtype=dt).reshape(want.shape)
            want = np.where(active, e, want)
        assert np.array_equal(fc.bits(g), fc.bits(np.ascontiguousarray(want))), n
    assert ngptot % nproma != 0                                # the shapes have a partial last block


# ---------------------------------------------------------------------------
# validation of a caller-owned set against the state API
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS, ids=PRECISION_IDS)
@pytest.mark.parametrize("col_offset", [0, 37])
@pytest.mark.parametrize("ngptot,nproma", [(1000, 64), (300, 64), (100, 100)])
def test_validate_matches_state(lib, hip, ds, ngptot, nproma, col_offset, precision):
    g = ca.GpuState(ds, ngptot, nproma, precision, col_offset=col_offset)
    df = ca.DeviceFields(ngptot, nproma, ds.klev, precision, place=False)
    try:
        g.run(ca.VARIANT_KSEG, 1)
        want = g.validate()
        df.expand(ds, col_offset)
        run_on(lib, hip, ds, df, ca.VARIANT_KSEG)
        got = df.validate(ds, col_offset)
    finally:
        g.close()
        df.close()
    for (name, key), x, y in zip(ca.VALIDATED, got, want):
        assert [cc.dbits(v) for v in x[:3]] == [cc.dbits(v) for v in y[:3]], (name, x, y)
        n = fc.rows_of(key, ds.klev) * ngptot
        assert_sums_close(x[3], x[5], y[3], y[5], n, name + " errsum")
        assert_sums_close(x[4], x[6], y[4], y[6], n, name + " refsum")


_TILED = {}   # (ngptot, col_offset): {key: (reference [rows][ngptot], exact sum of its magnitudes)}, computed once


def tiled_reference(ds, ngptot, col_offset):
    """Per validated field, ref[row][(col_offset + g) % klon] for g < ngptot and the exact sum of |ref|."""
    if (ngptot, col_offset) not in _TILED:
        cols = (col_offset + np.arange(ngptot)) % ds.klon
        tiled = {}
        for _, key in ca.VALIDATED:
            r = np.asarray(ds.reference[key], dtype=np.float64)
            r = np.ascontiguousarray(np.take(r.reshape(-1, r.shape[-1]), cols, axis=-1))
            tiled[key] = (r, cc.exact_sum(np.abs(r)))
        _TILED[(ngptot, col_offset)] = tiled
    return _TILED[(ngptot, col_offset)]


def restated_validation(v, r):
    """min v, max v, max |v - r| as NumPy has them and the exact sum of |v - r| (fields_compare_cases.restate)."""
    d = np.abs(v - r)
    return (float(np.fmin.reduce(v, axis=None)), float(np.fmax.reduce(v, axis=None)),
            float(np.fmax.reduce(d, axis=None, initial=0.0)), cc.exact_sum(d))


@pytest.mark.parametrize("precision", PRECISIONS, ids=PRECISION_IDS)
@pytest.mark.parametrize("col_offset", [0, 37])
@pytest.mark.parametrize("ngptot,nproma", [(300, 64), (100, 100)])
def test_validate_matches_host_restatement(lib, hip, ds, ngptot, nproma, col_offset, precision):
    """GpuState.validate() and DeviceFields.validate() run the same device code, so both are held to a
    restatement on the host from the downloaded outputs: min, max and max|d| bit for bit, the two sums
    against the exact rational sums (fields_compare_cases.assert_sum, n = rows * ngptot)."""
    g = ca.GpuState(ds, ngptot, nproma, precision, col_offset=col_offset)
    df = ca.DeviceFields(ngptot, nproma, ds.klev, precision, place=False)
    try:
        g.run(ca.VARIANT_KSEG, 1)
        state_stats = g.validate()
        state_out = g.outputs()
        df.expand(ds, col_offset)
        run_on(lib, hip, ds, df, ca.VARIANT_KSEG)
        fields_stats = df.validate(ds, col_offset)
        fields_out = {k: ca.blocks_to_columns(df.download_raw(k), ngptot) for _, k in ca.VALIDATED}   # no padding lanes
    finally:
        g.close()
        df.close()
    ref = tiled_reference(ds, ngptot, col_offset)
    for i, (name, key) in enumerate(ca.VALIDATED):
        r, refsum = ref[key]
        vs = np.ascontiguousarray(state_out[key], dtype=np.float64).reshape(r.shape)
        vf = np.ascontiguousarray(fields_out[key], dtype=np.float64).reshape(r.shape)
        assert r.shape == (fc.rows_of(key, ds.klev), ngptot)
        want_s = restated_validation(vs, r)
        want_f = want_s if np.array_equal(fc.bits(vs), fc.bits(vf)) else restated_validation(vf, r)
        for what, got, want in (("state", state_stats[i], want_s), ("fields", fields_stats[i], want_f)):
            assert want[3] is not None and refsum is not None, (what, name)
            assert [cc.dbits(x) for x in got[:3]] == [cc.dbits(x) for x in want[:3]], (what, name, got, want)
            cc.assert_sum(got[3], got[5], want[3], r.size, "%s %s errsum" % (what, name))
            cc.assert_sum(got[4], got[6], refsum, r.size, "%s %s refsum" % (what, name))


# ---------------------------------------------------------------------------
# the physics kernels held against each other through the comparison
# ---------------------------------------------------------------------------
def physics_set(lib, hip, ds, ngptot, nproma, precision, variant):
    df = ca.DeviceFields(ngptot, nproma, ds.klev, precision, place=False)
    df.expand(ds)
    run_on(lib, hip, ds, df, variant)
    return df


def test_kseg_against_kcache(lib, hip, ds):
    a = physics_set(lib, hip, ds, 300, 64, ca.FP64, ca.VARIANT_KSEG)
    b = physics_set(lib, hip, ds, 300, 64, ca.FP64, ca.VARIANT_KCACHE)
    try:
        got = a.compare(b, names=OUTPUTS)
    finally:
        a.close()
        b.close()
    assert sorted(got) == sorted(OUTPUTS)
    assert {n: g["mismatches"] for n, g in got.items() if g["mismatches"]} == {}
    assert all(g["compared"] == fc.rows_of(n, ds.klev) * 300 for n, g in got.items())


def test_kseg_against_packed_narrow_blocks(lib, hip, ds):
    a = physics_set(lib, hip, ds, 300, 64, ca.FP64, ca.VARIANT_KSEG)
    try:
        ca.narrow_pack(1)
        assert ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, 300, 16, ds.klev)["pack"] == 4
        b = physics_set(lib, hip, ds, 300, 16, ca.FP64, ca.VARIANT_KSEG)
    finally:
        ca.narrow_pack(-1)
    try:
        got = a.compare(b, names=OUTPUTS)
    finally:
        a.close()
        b.close()
    assert {n: g["mismatches"] for n, g in got.items() if g["mismatches"]} == {} and len(got) == 21


def test_fp64_against_mixed(lib, hip, ds):
    a = physics_set(lib, hip, ds, 300, 64, ca.FP64, ca.VARIANT_KSEG)
    b = physics_set(lib, hip, ds, 300, 24, ca.MIXED, ca.VARIANT_KSEG)
    try:
        dev = device_compare(lib, a, b, OUTPUTS)
        ha = ca.HostState(300, 64, ds.klev, ca.FP64, {n: a.download_raw(n) for n in OUTPUTS})
        hb = ca.HostState(300, 24, ds.klev, ca.MIXED, {n: b.download_raw(n) for n in OUTPUTS})
    finally:
        a.close()
        b.close()
    host = cc.new_diffs()
    fa, fb = ha.fields(), hb.fields()
    ca.check(lib.cloudsc_cpu_fields_compare(2, 300, ds.klev, ca.FP64, 64, C.byref(fa), ca.MIXED, 24, C.byref(fb), host))
    assert sum(dev[m].mismatches for m in range(len(fc.MEMBERS))) > 0       # float-rounded data: other bits
    assert_same_as_host(dev, host)


# ---------------------------------------------------------------------------
# the CLI on caller-owned fields
# ---------------------------------------------------------------------------
def validation_table(out):
    lines = out.splitlines()
    start = [i for i, ln in enumerate(lines) if "Variable" in ln and "MaxRelErr" in ln][0]
    return lines[start:]


@pytest.mark.parametrize("extra", [[], ["--precision", "mixed"]], ids=["fp64", "mixed"])
def test_cli_fields_caller(extra):
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    base = [exe, "1", "1000", "64"] + extra
    state = subprocess.run(base, capture_output=True, text=True, timeout=120)
    caller = subprocess.run(base + ["--fields", "caller"], capture_output=True, text=True, timeout=120)
    assert state.returncode == 0 and caller.returncode == 0, (state.stderr, caller.stderr)
    table = validation_table(caller.stdout)
    assert len(table) == 23 and table == validation_table(state.stdout)
