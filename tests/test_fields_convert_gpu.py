"""Field set conversion on the device (cloudsc_fields_convert): the cases of tests/test_fields_convert_cpu.py
compared on raw bits with the host form (itself held to the NumPy restatement there), and the physics run
through a re-blocked / narrowed field set against the unchanged state API."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca
import fields_convert_cases as fc
import mixed_expected as mx
from gpu_harness import lib, hip, run_on  # noqa: F401  (lib, hip: fixtures)

pytestmark = pytest.mark.gpu

INPUTS = list(ca.INPUT_FIELDS) + list(ca.INOUT_FIELDS)
OUTPUTS = [k for _, k in ca.VALIDATED]


def cpu_expected(lib, src, dnp, dp, names=None):
    """The host form's result on the same host arrays: a sentinel-filled HostSet after the conversion."""
    dst = fc.HostSet(src.ngptot, dnp, src.klev, dp, names=src.names)
    ca.check(lib.cloudsc_cpu_fields_convert(2, src.ngptot, src.klev, src.precision, src.nproma,
                                            C.byref(src.fields(names)), dp, dnp, C.byref(dst.fields(names))))
    return dst


def device_pair(src, dnp, dp):
    """src uploaded into a DeviceFields, and a destination DeviceFields filled with the sentinel."""
    a = ca.DeviceFields(src.ngptot, src.nproma, src.klev, src.precision, place=False, aerosols=True)
    b = ca.DeviceFields(src.ngptot, dnp, src.klev, dp, place=False, aerosols=True)
    a.upload(src.arrays)
    b.upload(fc.HostSet(src.ngptot, dnp, src.klev, dp, names=src.names).arrays)
    return a, b


def assert_same_bits(b, exp, names):
    for n in names:
        assert np.array_equal(fc.bits(b.download_raw(n).reshape(exp.arrays[n].shape)), fc.bits(exp.arrays[n])), n


# ---------------------------------------------------------------------------
# the shape table, the four storage pairs, ktype, sentinel and padding lanes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sp,dp", fc.STORAGE, ids=["d2d", "d2f", "f2d", "f2f"])
@pytest.mark.parametrize("ngptot,snp,dnp", fc.SHAPES)
def test_device_matches_cpu_form(lib, ngptot, snp, dnp, sp, dp):
    src = fc.HostSet(ngptot, snp, fc.KLEV, sp).fill_encoded()
    exp = cpu_expected(lib, src, dnp, dp)
    a, b = device_pair(src, dnp, dp)
    try:
        a.convert_to(b)
        assert_same_bits(b, exp, src.names)        # padding lanes of the last block included: still the sentinel
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("sp,dp", [(ca.FP64, ca.MIXED), (ca.MIXED, ca.FP64)], ids=["d2f", "f2d"])
def test_device_klev_137(lib, sp, dp):
    src = fc.HostSet(150, 24, 137, sp).fill_encoded()
    exp = cpu_expected(lib, src, 64, dp)
    a, b = device_pair(src, 64, dp)
    try:
        a.convert_to(b)
        assert_same_bits(b, exp, src.names)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("sp,dp", fc.STORAGE, ids=["d2d", "d2f", "f2d", "f2f"])
@pytest.mark.parametrize("snp,dnp", [(24, 64), (64, 24)])
def test_device_guard_margins(lib, hip, snp, dnp, sp, dp):
    """Destination arrays carved out of one sentinel-filled device buffer, each followed by a guard
    margin: after the conversion the whole buffer is the host form's arrays and untouched sentinel."""
    ngptot = 150
    src = fc.HostSet(ngptot, snp, fc.KLEV, sp).fill_encoded()
    exp = cpu_expected(lib, src, dnp, dp)
    a = ca.DeviceFields(ngptot, snp, fc.KLEV, sp, place=False, aerosols=True)
    arena = C.c_void_p()
    try:
        a.upload(src.arrays)
        offs, total = {}, 0
        for n in src.names:
            offs[n] = total
            total += (exp.arrays[n].nbytes + fc.GUARD * 8 + 255) // 256 * 256
        assert hip.hipMalloc(C.byref(arena), C.c_size_t(total)) == 0
        assert hip.hipMemset(arena, fc.SENTINEL_BYTE, C.c_size_t(total)) == 0
        df = ca.Fields()
        for n in src.names:
            setattr(df, n, arena.value + offs[n])
        ca.convert_fields(a.f, df, ngptot, fc.KLEV, sp, snp, dp, dnp)
        assert hip.hipDeviceSynchronize() == 0
        got = np.empty(total, dtype=np.uint8)
        assert hip.hipMemcpy(got.ctypes.data, arena, C.c_size_t(total), 2) == 0
        want = np.full(total, fc.SENTINEL_BYTE, dtype=np.uint8)
        for n in src.names:
            want[offs[n]:offs[n] + exp.arrays[n].nbytes] = np.ascontiguousarray(exp.arrays[n]).view(np.uint8).ravel()
        assert np.array_equal(got, want)
    finally:
        if arena.value:
            hip.hipFree(arena)
        a.close()


def test_device_narrowing_edges(lib):
    v = fc.narrowing_edges()
    n = v.size
    src = fc.HostSet(n, n, 2, ca.FP64, names=["pt"])
    src.arrays["pt"][0, 0, :] = v
    src.arrays["pt"][0, 1, :] = v[::-1]
    exp = cpu_expected(lib, src, 4, ca.MIXED)
    a, b = device_pair(src, 4, ca.MIXED)
    try:
        a.convert_to(b, names=["pt"])
        got = b.download_raw("pt")
    finally:
        a.close()
        b.close()
    want = exp.arrays["pt"]
    cols = fc.to_columns(want, n)
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(fc.bits(cols[0][~np.isnan(v)]), fc.bits(v.astype(np.float32)[~np.isnan(v)]))
    nan = np.isnan(want)
    assert np.count_nonzero(nan) == 2 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(fc.bits(got)[~nan], fc.bits(want)[~nan])


def test_device_subset(lib):
    src = fc.HostSet(150, 24, fc.KLEV, ca.FP64).fill_encoded()
    exp = cpu_expected(lib, src, 64, ca.MIXED, names=["pt", "pclv"])
    a, b = device_pair(src, 64, ca.MIXED)
    try:
        a.convert_to(b, names=["pt", "pclv"])
        assert_same_bits(b, exp, src.names)        # every other member still the sentinel
    finally:
        a.close()
        b.close()


def test_non_default_stream(lib, hip):
    src = fc.HostSet(150, 24, fc.KLEV, ca.FP64).fill_encoded()
    exp = cpu_expected(lib, src, 64, ca.MIXED)
    a, b = device_pair(src, 64, ca.MIXED)
    st = C.c_void_p()
    got = {}
    try:
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipStreamCreateWithFlags(C.byref(st), C.c_uint(1)) == 0      # hipStreamNonBlocking
        a.convert_to(b, stream=st)
        assert hip.hipStreamSynchronize(st) == 0
        for n in src.names:      # read with plain copies after the stream's own sync
            got[n] = np.empty_like(exp.arrays[n])
            assert hip.hipMemcpy(got[n].ctypes.data, getattr(b.f, n), C.c_size_t(got[n].nbytes), 2) == 0
    finally:
        if st.value:
            hip.hipStreamDestroy(st)
        a.close()
        b.close()
    for n in src.names:
        assert np.array_equal(fc.bits(got[n]), fc.bits(exp.arrays[n])), n


# ---------------------------------------------------------------------------
# the physics through converted field sets
# ---------------------------------------------------------------------------
def state_inputs(lib, g):
    """The device pointers of a state's input fields, plude restored from its pristine copy."""
    g.reset()
    g.sync()
    f = ca.Fields()
    ca.check(lib.cloudsc_state_fields(g.h, C.byref(f)))
    return ca.fields_subset(f, INPUTS)


def test_physics_through_a_reblock(lib, hip, ds):
    """fp64 KSEG on a state at NPROMA 24, and on its inputs re-blocked to NPROMA 64 with the outputs
    converted back to NPROMA 24: the 21 validated fields bit for bit (columns are independent)."""
    n, klev = 300, ds.klev
    g = ca.GpuState(ds, n, 24, ca.FP64)
    d64 = ca.DeviceFields(n, 64, klev, ca.FP64, place=False)
    d24 = ca.DeviceFields(n, 24, klev, ca.FP64, place=False)
    try:
        g.run(ca.VARIANT_KSEG, 1)
        want = {k: g.download(k) for k in OUTPUTS}
        ca.convert_fields(state_inputs(lib, g), ca.fields_subset(d64.f, INPUTS), n, klev, ca.FP64, 24, ca.FP64, 64)
        run_on(lib, hip, ds, d64, ca.VARIANT_KSEG)
        d64.convert_to(d24, names=OUTPUTS)
        got = {k: d24.download_raw(k) for k in OUTPUTS}
    finally:
        g.close()
        d64.close()
        d24.close()
    for k in OUTPUTS:
        a, b = ca.blocks_to_columns(got[k], n), ca.blocks_to_columns(want[k], n)
        assert a.dtype == np.float64 and np.array_equal(fc.bits(a), fc.bits(b)), k


def test_mixed_from_doubles(lib, hip, ds):
    """fp64 inputs at NPROMA 32 narrowed into a CLOUDSC_MIXED set at NPROMA 64: KSEG mixed gives the bits
    of a CLOUDSC_MIXED state made from the same dataset (expansion and conversion narrow alike)."""
    n, klev = 300, ds.klev
    g = ca.GpuState(ds, n, 32, ca.FP64)
    dm = ca.DeviceFields(n, 64, klev, ca.MIXED, place=False)
    gm = ca.GpuState(ds, n, 64, ca.MIXED)
    try:
        ca.convert_fields(state_inputs(lib, g), ca.fields_subset(dm.f, INPUTS), n, klev, ca.FP64, 32, ca.MIXED, 64)
        run_on(lib, hip, ds, dm, ca.VARIANT_KSEG)
        got = {k: ca.blocks_to_columns(dm.download(k), n) for k in OUTPUTS}
        gm.run(ca.VARIANT_KSEG, 1)
        want = {k: mx.as_f32(v) for k, v in gm.outputs().items()}
    finally:
        g.close()
        dm.close()
        gm.close()
    assert mx.mismatches(got, want) == {}


def test_reference_driver_shape(lib, hip, ds):
    """cloudsc_fields_alloc with its placement search, filled by conversion from a flat
    (nproma = ngptot) fp64 upload, KCACHE at NPROMA 64: the state API's bits."""
    n, klev = 300, ds.klev
    flat = ca.DeviceFields(n, n, klev, ca.FP64, place=False)
    df = ca.DeviceFields(n, 64, klev, ca.FP64)
    g = ca.GpuState(ds, n, 64, ca.FP64)
    try:
        host = ca.make_host_state(ds, n, n, ca.FP64)
        flat.upload({k: host.arrays[k] for k in INPUTS})
        flat.convert_to(df, names=INPUTS)
        run_on(lib, hip, ds, df, ca.VARIANT_KCACHE)
        got = {k: ca.blocks_to_columns(df.download_raw(k), n) for k in OUTPUTS}
        g.run(ca.VARIANT_KCACHE, 1)
        want = g.outputs()
    finally:
        flat.close()
        df.close()
        g.close()
    for k in OUTPUTS:
        assert np.array_equal(fc.bits(got[k]), fc.bits(np.ascontiguousarray(want[k]))), k
