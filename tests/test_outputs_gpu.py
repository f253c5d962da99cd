"""The output selection on the device: cloudsc_gpu_run_outputs(CLOUDSC_OUTPUTS_PROGNOSTIC) against
cloudsc_gpu_run on a second set holding the same inputs, on raw bits over the eleven kept outputs -- on the
device (cloudsc_fields_compare, the ten diagnostic fluxes NULL in both operands) and again on the host,
where the sentinel bytes of padding lanes and of non-NULL diagnostic members are checked too; fp64 also
against the oracle -- and cloudsc_fields_alloc_outputs."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca

pytestmark = pytest.mark.gpu

DIAG = ca.DIAGNOSTIC_FLUX_FIELDS
KEPT = ca.selected_outputs(ca.OUTPUTS_PROGNOSTIC)
ALL21 = ca.selected_outputs(ca.OUTPUTS_ALL)
PATTERN = 0xC3
PRECISIONS = {"fp64": ca.FP64, "fp32": ca.FP32, "mixed": ca.MIXED}
VARIANTS = {"kcache": ca.VARIANT_KCACHE, "kseg": ca.VARIANT_KSEG}
# partial last block | two sub-blocks per block under KSEG | packed by default | packed on request | one wide block
SHAPES = [(300, 64), (200, 128), (100, 16), (70, 32), (300, 300)]


@pytest.fixture(scope="module")
def lib():
    lib = ca.gpu_lib()
    assert ca.device_count() > 0
    return lib


@pytest.fixture(scope="module")
def hip():
    h = ca._hip()
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    return h


@pytest.fixture(autouse=True)
def restore_knobs():
    yield
    ca.narrow_pack(-1)
    ca.kseg_schedule(0, 0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def columns(blocks, ngptot):
    return np.ascontiguousarray(ca.blocks_to_columns(blocks, ngptot))


def host_inputs(ds, ngptot, nproma, precision):
    """Block-layout host arrays with every output (and plude's padding lanes) set to a byte pattern."""
    st = ca.make_host_state(ds, ngptot, nproma, precision)
    nb = ca.nblocks_of(ngptot, nproma)
    out = {}
    for name, a in st.arrays.items():
        a = np.ascontiguousarray(a).copy()
        if name in ca.OUTPUT_FIELDS:
            a.view(np.uint8)[...] = PATTERN
        if name == "plude":
            tail = ngptot - (nb - 1) * nproma
            a[nb - 1, ..., tail:].view(np.uint8)[...] = PATTERN
        out[name] = a
    return out


_oracle = {}


def oracle_columns(oracle_mod, ds, key, ngptot, nproma):
    """The fp64 oracle's outputs as columns, once per (dataset, shape), read-only."""
    k = (key, ngptot, nproma)
    if k not in _oracle:
        ost, _ = oracle_mod.run_oracle(ds, ngptot, nproma)
        _oracle[k] = {n: columns(ost.arrays[n], ngptot) for n in ALL21}
        for a in _oracle[k].values():
            a.setflags(write=False)
    return _oracle[k]


class Sets:
    """One problem on the device in several sets with the same inputs and pattern-filled outputs: "all"
    (cloudsc_fields_alloc), "null" (cloudsc_fields_alloc_outputs(PROGNOSTIC): the ten members NULL) and "kept"
    (all 21 allocated, run with PROGNOSTIC: the ten must keep the pattern)."""

    def __init__(self, lib, hip, ds, ngptot, nproma, precision, which=("all", "null", "kept")):
        self.lib, self.hip, self.ds = lib, hip, ds
        self.ngptot, self.nproma, self.precision = ngptot, nproma, precision
        self.aer = bool(ds.params.get("laericesed") or ds.params.get("laericeauto"))
        self.host = host_inputs(ds, ngptot, nproma, precision)
        self.ws = C.c_void_p()
        self.sets = {}
        for w in which:
            outputs = ca.OUTPUTS_PROGNOSTIC if w == "null" else ca.OUTPUTS_ALL
            self.sets[w] = ca.DeviceFields(ngptot, nproma, ds.klev, precision, place=False, aerosols=self.aer,
                                           outputs=outputs)
            self.sets[w].upload(self.host)
        p = ca.Params.from_dict(ds.params)
        ca.check(lib.cloudsc_gpu_init(0, C.byref(p)))

    def scratch(self, variant):
        if variant & 0xff == ca.VARIANT_KSEG and not self.ws.value:
            nbytes = self.lib.cloudsc_gpu_scratch_bytes(self.precision, ca.VARIANT_KSEG, self.ngptot, self.nproma,
                                                        self.ds.klev)
            assert nbytes > 0
            assert self.hip.hipMalloc(C.byref(self.ws), C.c_size_t(nbytes)) == 0
            assert self.hip.hipMemset(self.ws, 0, C.c_size_t(256)) == 0
        return self.ws

    def run(self, which, variant, outputs, stream=None):
        """One step on a set (cloudsc_gpu_run for outputs None), followed by its check."""
        ws = self.scratch(variant)
        f = self.sets[which].f
        if outputs is None:
            ca.check(self.lib.cloudsc_gpu_run(0, stream, self.precision, variant, self.ngptot, self.nproma,
                                              self.ds.klev, C.byref(f), ws))
        else:
            ca.gpu_run_outputs(f, self.precision, variant, outputs, self.ngptot, self.nproma, self.ds.klev, scratch=ws,
                               stream=stream)
        assert self.lib.cloudsc_gpu_check(0, stream, variant & 0xff, ws) == 0

    def device_mismatches(self, which, names=KEPT, against="all", stream=None):
        """cloudsc_fields_compare of `names` of a set against the "all" set's: {member: mismatches} where not 0."""
        a = ca.fields_subset(self.sets[which].f, names)
        b = ca.fields_subset(self.sets[against].f, names)
        if names is KEPT:
            assert not any(getattr(a, n) or getattr(b, n) for n in DIAG)    # NULL in both operands
        d = ca.compare_fields(a, b, self.ngptot, self.ds.klev, self.precision, self.nproma, self.precision,
                              self.nproma, stream=stream)
        assert sorted(d) == sorted(names)
        assert all(v["compared"] > 0 for v in d.values())
        return {k: v["mismatches"] for k, v in d.items() if v["mismatches"]}

    def host_check(self, which, names=KEPT, against="all", oracle=None):
        """The same on the host, whole arrays (padding lanes included), and the pattern bytes: padding lanes
        of every output, and every byte of a diagnostic member that was not to be written."""
        self.hip.hipDeviceSynchronize()
        wrong = []
        tail = self.ngptot % self.nproma
        for k in names:
            got, ref = self.sets[which].download_raw(k), self.sets[against].download_raw(k)
            if not np.array_equal(bits(got), bits(ref)):
                wrong.append("%s: differs (padding included)" % k)
            if tail and not (bits(got[-1][..., tail:]) == PATTERN).all():
                wrong.append("%s: a padding lane was written" % k)
            if oracle is not None and not np.array_equal(bits(columns(got, self.ngptot)), bits(oracle[k])):
                wrong.append("%s: differs from the oracle" % k)
        if names is KEPT:
            for k in DIAG:
                if getattr(self.sets[which].f, k) and not (bits(self.sets[which].download_raw(k)) == PATTERN).all():
                    wrong.append("%s: written by a PROGNOSTIC run" % k)
        return wrong

    def close(self):
        if self.ws.value:
            self.hip.hipFree(self.ws)
            self.ws = C.c_void_p()
        for s in self.sets.values():
            s.close()


def prognostic_parity(s, variant, oracle=None, stream=None, run_all=True):
    """cloudsc_gpu_run on "all" (run_all False: the caller has run it), PROGNOSTIC on "null" and "kept"; the
    eleven kept members on the device and on the host."""
    if run_all:
        s.run("all", variant, None, stream)
    for w in ("null", "kept"):
        s.run(w, variant, ca.OUTPUTS_PROGNOSTIC, stream)
        assert not any(getattr(s.sets["null"].f, n) for n in DIAG)
        assert all(getattr(s.sets["kept"].f, n) for n in DIAG)
        assert s.device_mismatches(w, stream=stream) == {}, w
        assert s.host_check(w, oracle=oracle) == [], w
    # the step did something: the reference run wrote the diagnostic fluxes and the kept outputs
    assert not (bits(s.sets["all"].download_raw("pfsqlf")) == PATTERN).all()
    assert not (bits(s.sets["null"].download_raw("pfplsn")) == PATTERN).all()


CASES = [(n, p, v) for (n, p) in SHAPES for v in VARIANTS if not (p > 256 and v == "kcache")]


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
        df.upload(host_inputs(ds, ngptot, nproma, ca.FP64))
        p = ca.Params.from_dict(ds.params)
        ca.check(lib.cloudsc_gpu_init(0, C.byref(p)))
        nbytes = lib.cloudsc_gpu_scratch_bytes(ca.FP64, ca.VARIANT_KSEG, ngptot, nproma, ds.klev)
        assert hip.hipMalloc(C.byref(ws), C.c_size_t(nbytes)) == 0
        assert hip.hipMemset(ws, 0, C.c_size_t(256)) == 0
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
        df.upload(host_inputs(ds, ngptot, nproma, ca.FP64))
        p = ca.Params.from_dict(ds.params)
        ca.check(lib.cloudsc_gpu_init(0, C.byref(p)))
        nbytes = lib.cloudsc_gpu_scratch_bytes(ca.FP64, ca.VARIANT_KSEG, ngptot, nproma, ds.klev)
        assert hip.hipMalloc(C.byref(ws), C.c_size_t(nbytes)) == 0
        assert hip.hipMemset(ws, 0, C.c_size_t(256)) == 0
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
