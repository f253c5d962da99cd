"""The output selection on the device: cloudsc_gpu_run_outputs(CLOUDSC_OUTPUTS_PROGNOSTIC) against
cloudsc_gpu_run on a second set holding the same inputs, on raw bits over the eleven kept outputs -- on the
device (cloudsc_fields_compare, the ten diagnostic fluxes NULL in both operands) and again on the host,
where the sentinel bytes of padding lanes and of non-NULL diagnostic members are checked too; fp64 also
against the oracle -- and cloudsc_fields_alloc_outputs."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca
from gpu_harness import ALL21, CASES, DIAG, KEPT, PATTERN, PRECISIONS, VARIANTS
from gpu_harness import Sets, columns, host_inputs, init_params, kseg_workspace, oracle_columns, prognostic_parity
from gpu_harness import raw_bits as bits
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("ngptot,nproma,variant", CASES)
def test_run_outputs_prognostic_bitwise(lib, hip, ds, oracle_mod, ngptot, nproma, variant, precision):
    s = Sets(lib, hip, ds, ngptot, nproma, PRECISIONS[precision])
    try:
        if nproma == 32:
            ca.narrow_pack(1)
        geo = ca.launch_geometry(PRECISIONS[precision], VARIANTS[variant], ngptot, nproma, ds.klev)
        assert geo["pack"] == (64 // nproma if nproma <= 32 else 1)
        oracle = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma) if precision == "fp64" else None
        prognostic_parity(s, VARIANTS[variant], oracle)
    finally:
        s.close()


def test_run_outputs_aerosols(lib, hip, ds, oracle_mod):
    import make_fixtures as mf
    a = mf.with_aerosols(ds)
    for variant, nproma in ((ca.VARIANT_KSEG, 64), (ca.VARIANT_KCACHE, 16)):
        s = Sets(lib, hip, a, 100, nproma, ca.FP64)
        try:
            assert s.aer
            prognostic_parity(s, variant, oracle_columns(oracle_mod, a, "aerosol", 100, nproma))
        finally:
            s.close()


def test_run_outputs_non_default_stream(lib, hip, ds):
    s = Sets(lib, hip, ds, 200, 128, ca.MIXED)
    st = C.c_void_p()
    try:
        assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0       # hipStreamNonBlocking
        hip.hipDeviceSynchronize()                                    # the uploads (null stream) are done
        prognostic_parity(s, ca.VARIANT_KSEG, stream=st)
    finally:
        if st.value:
            hip.hipStreamSynchronize(st)
            hip.hipStreamDestroy(st)
        s.close()


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_run_outputs_three_segment_hand_off(lib, hip, ds, oracle_mod, precision):
    """3 segments on 3 workgroups: every column's carried state crosses the workspace twice, without the six
    flux planes in the PROGNOSTIC launches."""
    s = Sets(lib, hip, ds, 300, 64, PRECISIONS[precision])
    try:
        ca.kseg_schedule(3, 3)
        oracle = oracle_columns(oracle_mod, ds, "ds", 300, 64) if precision == "fp64" else None
        prognostic_parity(s, ca.VARIANT_KSEG, oracle)
    finally:
        s.close()


def test_run_outputs_shares_a_workspace(lib, hip, ds, oracle_mod):
    """ALL, then PROGNOSTIC, then ALL on one KSEG workspace that is zeroed once, before the first launch: the
    workspace keeps its 19-plane layout, so every launch is correct whatever ran before it."""
    s = Sets(lib, hip, ds, 300, 64, ca.FP64, which=("all", "null", "kept"))
    try:
        ca.kseg_schedule(3, 0)                   # more hand-offs than the default's one
        oracle = oracle_columns(oracle_mod, ds, "ds", 300, 64)
        s.run("all", ca.VARIANT_KSEG, ca.OUTPUTS_ALL)
        s.run("null", ca.VARIANT_KSEG, ca.OUTPUTS_PROGNOSTIC)
        s.run("kept", ca.VARIANT_KSEG, ca.OUTPUTS_ALL)          # the "kept" set, all 21 written this time
        assert s.device_mismatches("null") == {}
        assert s.device_mismatches("kept", names=ALL21) == {}
        assert s.host_check("all", names=ALL21, oracle=oracle) == []
        assert s.host_check("null", oracle=oracle) == []
        assert s.host_check("kept", names=ALL21, oracle=oracle) == []
    finally:
        s.close()


def test_run_outputs_all_is_gpu_run(lib, hip, ds):
    s = Sets(lib, hip, ds, 300, 64, ca.FP32, which=("all", "kept"))
    try:
        for variant in (ca.VARIANT_KSEG, ca.VARIANT_KCACHE, ca.VARIANT_SCC_PRIVATE,
                        ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM):
            for w in s.sets.values():
                w.upload(s.host)
            s.run("all", variant, None)
            s.run("kept", variant, ca.OUTPUTS_ALL)
            assert s.device_mismatches("kept", names=ALL21) == {}
            assert s.host_check("kept", names=ALL21) == []
        # and the forms PROGNOSTIC does not have, on real sets
        ws = s.scratch(ca.VARIANT_KSEG)
        for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM):
            assert lib.cloudsc_gpu_run_outputs(0, None, ca.FP32, variant, ca.OUTPUTS_PROGNOSTIC, 300, 64, ds.klev,
                                               C.byref(s.sets["kept"].f), ws) == ca.EINVAL
    finally:
        s.close()


# ---------------------------------------------------------------------------
# cloudsc_fields_alloc_outputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("place", [False, True], ids=["place_none", "placed"])
def test_fields_alloc_outputs_prognostic(lib, hip, ds, oracle_mod, place):
    ngptot, nproma = 300, 64
    df = ca.DeviceFields(ngptot, nproma, ds.klev, ca.FP64, place=place, outputs=ca.OUTPUTS_PROGNOSTIC)
    ws = C.c_void_p()
    try:
        assert not any(getattr(df.f, n) for n in DIAG)
        assert all(getattr(df.f, n) for n in list(ca.INPUT_FIELDS) + list(KEPT))
        assert not any(getattr(df.f, n) for n in ca.AEROSOL_FIELDS)
        r = df.report.to_dict()
        if place:
            assert r["method"] == "rw-probe" and r["launches"] >= 30 and r["search_ms"] > 0, r
            assert 0 < r["probe_final_ms"] <= r["probe_first_ms"] and 0 <= r["moves"] <= r["tries"], r
            assert len(KEPT) <= r["tries"] <= 8 * len(KEPT) + 2 * len(KEPT), r     # sets of eleven, not of 21
            assert 0 < r["peak_transient_bytes"] <= r["transient_budget_bytes"], r
        else:
            assert r["method"] == "none" and r["launches"] == 0 and r["tries"] == 0, r
        df.upload(host_inputs(ds, ngptot, nproma, ca.FP64, PATTERN))
        init_params(lib, ds.params)
        ws = kseg_workspace(lib, hip, ca.FP64, ca.VARIANT_KSEG, ngptot, nproma, ds.klev)
        # the step of cloudsc_gpu_run needs the ten members this set does not have
        assert lib.cloudsc_gpu_run(0, None, ca.FP64, ca.VARIANT_KSEG, ngptot, nproma, ds.klev, C.byref(df.f),
                                   ws) == ca.EINVAL
        ca.gpu_run_outputs(df.f, ca.FP64, ca.VARIANT_KSEG, ca.OUTPUTS_PROGNOSTIC, ngptot, nproma, ds.klev, scratch=ws)
        assert lib.cloudsc_gpu_check(0, None, ca.VARIANT_KSEG, ws) == 0
        oracle = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma)
        for k in KEPT:
            got = df.download_raw(k)
            assert np.array_equal(bits(columns(got, ngptot)), bits(oracle[k])), k
            assert (bits(got[-1][..., ngptot % nproma:]) == PATTERN).all(), k
        f = df.f
        assert lib.cloudsc_fields_free(0, C.byref(f)) == 0
        assert not any(getattr(f, n) for n in ca.ALL_FIELDS)
    finally:
        if ws.value:
            hip.hipFree(ws)
        df.close()


def test_fields_alloc_outputs_all_is_fields_alloc(lib, hip, ds, oracle_mod):
    ngptot, nproma = 300, 64
    f, r = ca.Fields(), ca.Placement()
    ca.check(lib.cloudsc_fields_alloc_outputs(0, ca.FP64, ngptot, nproma, ds.klev, ca.PLACE_NONE, ca.OUTPUTS_ALL,
                                              C.byref(f), C.byref(r)))
    ws = C.c_void_p()
    try:
        assert all(getattr(f, n) for n in list(ca.INPUT_FIELDS) + list(ALL21))
        assert not any(getattr(f, n) for n in ca.AEROSOL_FIELDS)
        df = ca.DeviceFields.__new__(ca.DeviceFields)      # the upload / download helpers on this set
        df.lib, df.hip, df.f, df.tend_planes = lib, hip, f, 0
        df.ngptot, df.nproma, df.klev, df.precision, df.device = ngptot, nproma, ds.klev, ca.FP64, 0
        df.upload(host_inputs(ds, ngptot, nproma, ca.FP64, PATTERN))
        init_params(lib, ds.params)
        ws = kseg_workspace(lib, hip, ca.FP64, ca.VARIANT_KSEG, ngptot, nproma, ds.klev)
        ca.check(lib.cloudsc_gpu_run(0, None, ca.FP64, ca.VARIANT_KSEG, ngptot, nproma, ds.klev, C.byref(f), ws))
        assert lib.cloudsc_gpu_check(0, None, ca.VARIANT_KSEG, ws) == 0
        oracle = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma)
        for k in ALL21:
            assert np.array_equal(bits(columns(df.download_raw(k), ngptot)), bits(oracle[k])), k
    finally:
        if ws.value:
            hip.hipFree(ws)
        assert lib.cloudsc_fields_free(0, C.byref(f)) == 0
    assert not f.pt and not f.pfsqlf and not f.pfhpsn
