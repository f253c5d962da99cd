"""Packed tendency buffers on the device: cloudsc_gpu_run_tendbuf against
cloudsc_gpu_run on separate arrays holding the same inputs (itself pinned to the
oracle elsewhere), on raw bits over the 20 outputs and plude -- on the device
(unpack, then cloudsc_fields_compare) and again on the host, where the
buffers' sentinel bytes in unbound planes and padding lanes are checked too --
and cloudsc_fields_convert_tendbuf against its host twin."""
import ctypes as C
import os
import subprocess

import pytest

import cloudsc_amd as ca
import host_harness as tc
from gpu_harness import CASES, DeviceSide, PRECISIONS, Pair, VARIANTS, validation_table
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SETTINGS = [(8, "reference"), (11, "permuted")]


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("ngptot,nproma,variant", CASES)
def test_run_tendbuf_bitwise(lib, hip, ds, ngptot, nproma, variant, precision):
    for tend_planes, order in SETTINGS:
        pr = Pair(lib, hip, ds, ngptot, nproma, PRECISIONS[precision], tend_planes, order)
        try:
            if nproma == 32:
                ca.narrow_pack(1)
            geo = ca.launch_geometry(PRECISIONS[precision], VARIANTS[variant], ngptot, nproma, ds.klev)
            assert geo["pack"] == (64 // nproma if nproma <= 32 else 1)
            pr.fill()
            pr.run_both(VARIANTS[variant])
            assert pr.device_mismatches() == {}
            assert pr.host_check() == []
        finally:
            pr.close()


@pytest.mark.parametrize("tend_planes,order", [(8, "permuted"), (11, "reference")])
def test_run_tendbuf_other_settings(lib, hip, ds, tend_planes, order):
    pr = Pair(lib, hip, ds, 300, 64, ca.FP64, tend_planes, order)
    try:
        pr.fill()
        pr.run_both(ca.VARIANT_KSEG)
        assert pr.device_mismatches() == {}
        assert pr.host_check() == []
    finally:
        pr.close()


def test_run_tendbuf_aerosols(lib, hip, ds):
    import make_fixtures as mf
    s = mf.with_aerosols(ds)
    for variant, nproma in ((ca.VARIANT_KSEG, 64), (ca.VARIANT_KCACHE, 16)):
        pr = Pair(lib, hip, s, 100, nproma, ca.FP64, 11, "permuted")
        try:
            assert pr.aer
            pr.fill()
            pr.run_both(variant)
            assert pr.device_mismatches() == {}
            assert pr.host_check() == []
        finally:
            pr.close()


def test_run_tendbuf_refuses_fp32_exact_libm(lib, hip, ds):
    pr = Pair(lib, hip, ds, 100, 16, ca.FP32, 8, "reference")
    try:
        for variant in (ca.VARIANT_KSEG, ca.VARIANT_KCACHE):
            assert lib.cloudsc_gpu_run_tendbuf(0, None, ca.FP32, variant | ca.FP32_EXACT_LIBM, 100, 16, ds.klev, 8,
                                               C.byref(pr.packed.f), C.c_void_p(0x100)) == ca.EINVAL
    finally:
        pr.close()


def test_run_tendbuf_non_default_stream(lib, hip, ds):
    pr = Pair(lib, hip, ds, 200, 128, ca.MIXED, 11, "permuted")
    st = C.c_void_p()
    try:
        assert hip.hipStreamCreateWithFlags(C.byref(st), C.c_uint(1)) == 0      # hipStreamNonBlocking
        pr.fill()
        hip.hipDeviceSynchronize()
        pr.run_both(ca.VARIANT_KSEG, stream=st)
        assert pr.device_mismatches(stream=st) == {}
        assert hip.hipStreamSynchronize(st) == 0
        assert pr.host_check() == []
    finally:
        if st.value:
            hip.hipStreamDestroy(st)
        pr.close()


def test_run_tendbuf_few_workgroups_many_handoffs(lib, hip, ds):
    pr = Pair(lib, hip, ds, 300, 64, ca.FP64, 8, "reference")
    try:
        ca.kseg_schedule(3, 3)
        pr.fill()
        pr.run_both(ca.VARIANT_KSEG)
        assert pr.device_mismatches() == {}
        assert pr.host_check() == []
    finally:
        pr.close()


def test_run_tendbuf_refuses_scc(lib, hip, ds):
    pr = Pair(lib, hip, ds, 100, 64, ca.FP64, 8, "reference")
    try:
        for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE):
            assert lib.cloudsc_gpu_run_tendbuf(0, None, ca.FP64, variant, 100, 64, ds.klev, 8, C.byref(pr.packed.f),
                                               C.c_void_p(0x100)) == ca.EINVAL
    finally:
        pr.close()


# ---------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("common,planes", [([], []), (["--variant", "kcache", "--precision", "mixed"],
                                                     ["--tend-planes", "11"])], ids=["default", "planes11_kcache_mixed"])
def test_cli_fields_tendbuf(common, planes):
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    base = [exe, "1", "300", "64"] + common
    caller = subprocess.run(base + ["--fields", "caller"], capture_output=True, text=True, timeout=120)
    tendbuf = subprocess.run(base + ["--fields", "tendbuf"] + planes, capture_output=True, text=True, timeout=120)
    assert caller.returncode == 0 and tendbuf.returncode == 0, (caller.stderr, tendbuf.stderr)
    table = validation_table(tendbuf.stdout)
    assert len(table) == 23 and table == validation_table(caller.stdout)


# ---------------------------------------------------------------------------
# the device conversion against the host twin
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(tc.CONV_CASES))
def test_device_convert_tendbuf_against_host_twin(lib, hip, case):
    s, d = tc.CONV_CASES[case]
    src, dst = tc.Side(*s), tc.Side(*d, values=False)
    dsrc, ddst = DeviceSide(hip, src), DeviceSide(hip, dst)
    try:
        ca.convert_fields_tendbuf(dsrc.f, ddst.f, src.ngptot, tc.CONV_KLEV, src.precision, src.nproma,
                                  src.tend_planes, dst.precision, dst.nproma, dst.tend_planes)
        tc.convert(src, dst)
        assert tc.same_storage(ddst.snapshot(), dst.snapshot())
        assert tc.same_storage(dsrc.snapshot(), src.snapshot())
    finally:
        dsrc.close()
        ddst.close()


def test_device_convert_tendbuf_zero_planes_is_convert(lib, hip):
    src = tc.Side(ca.FP64, 24, 0)
    a, b = tc.Side(ca.MIXED, 64, 0, values=False), tc.Side(ca.MIXED, 64, 0, values=False)
    dsrc, da, db = DeviceSide(hip, src), DeviceSide(hip, a), DeviceSide(hip, b)
    try:
        ca.convert_fields_tendbuf(dsrc.f, da.f, src.ngptot, tc.CONV_KLEV, src.precision, src.nproma, 0, a.precision,
                                  a.nproma, 0)
        ca.convert_fields(dsrc.f, db.f, src.ngptot, tc.CONV_KLEV, src.precision, src.nproma, b.precision, b.nproma)
        assert tc.same_storage(da.snapshot(), db.snapshot())
        tc.convert(src, a)
        assert tc.same_storage(da.snapshot(), a.snapshot())
    finally:
        for x in (dsrc, da, db):
            x.close()
