"""Packed tendency buffers on the device: cloudsc_gpu_run_tendbuf against
cloudsc_gpu_run on separate arrays holding the same inputs (itself pinned to the
oracle elsewhere), on raw bits over the 20 outputs and plude -- on the device
(unpack, then cloudsc_fields_compare) and again on the host, where the
buffers' sentinel bytes in unbound planes and padding lanes are checked too --
and cloudsc_fields_convert_tendbuf against its host twin."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import tendbuf_cases as tb
import test_tendbuf_cpu as tc

pytestmark = pytest.mark.gpu

NAMES = [k for _, k in ca.VALIDATED]
PATTERN = 0xC3
PRECISIONS = {"fp64": ca.FP64, "fp32": ca.FP32, "mixed": ca.MIXED}
VARIANTS = {"kcache": ca.VARIANT_KCACHE, "kseg": ca.VARIANT_KSEG}
SETTINGS = [(8, "reference"), (11, "permuted")]


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


def host_inputs(ds, ngptot, nproma, precision):
    """Block-layout host arrays with every output (and plude's padding lanes) set to a byte pattern."""
    st = ca.make_host_state(ds, ngptot, nproma, precision)
    nb = ca.nblocks_of(ngptot, nproma)
    out = {}
    for name, a in st.arrays.items():
        a = np.ascontiguousarray(a).copy()
        if name in ca.OUTPUT_FIELDS and name != "plude":
            a.view(np.uint8)[...] = PATTERN
        if name == "plude":
            tail = ngptot - (nb - 1) * nproma
            a[nb - 1, ..., tail:].view(np.uint8)[...] = PATTERN
        out[name] = a
    return out


class Pair:
    """One problem twice on the device: `plain` with separate tendency arrays, `packed` with the two
    tendency buffers of DeviceFields(tend_planes=...)."""

    def __init__(self, lib, hip, ds, ngptot, nproma, precision, tend_planes, order):
        self.lib, self.hip, self.ds = lib, hip, ds
        self.ngptot, self.nproma, self.precision, self.tend_planes = ngptot, nproma, precision, tend_planes
        self.nb = ca.nblocks_of(ngptot, nproma)
        self.aer = bool(ds.params.get("laericesed") or ds.params.get("laericeauto"))
        self.host = host_inputs(ds, ngptot, nproma, precision)
        self.lay = tb.layout(order, tend_planes)
        self.plain = ca.DeviceFields(ngptot, nproma, ds.klev, precision, place=False, aerosols=self.aer)
        self.packed = ca.DeviceFields(ngptot, nproma, ds.klev, precision, place=False, aerosols=self.aer,
                                      tend_planes=tend_planes)
        self.ws = C.c_void_p()
        dt = ca.storage_dtype(precision)
        self.buf_tmp = tb.empty_buffer(self.nb, tend_planes, ds.klev, nproma, dt, tb.SENTINEL_TMP)
        self.buf_loc = tb.empty_buffer(self.nb, tend_planes, ds.klev, nproma, dt, tb.SENTINEL_LOC)
        for n in tb.TMP:
            tb.put(self.buf_tmp, self.lay[n], self.host[n], ngptot)
        assert self.buf_tmp.nbytes == self.packed.tendbuf_nbytes()
        if order != "reference":       # the constructor bound the reference's planes
            plane = ds.klev * nproma * self.buf_tmp.itemsize
            for names, base in ((tb.TMP, self.packed.buffer_tmp), (tb.LOC, self.packed.buffer_loc)):
                for n in names:
                    setattr(self.packed.f, n, base + self.lay[n] * plane)
        p = ca.Params.from_dict(ds.params)
        ca.check(lib.cloudsc_gpu_init(0, C.byref(p)))

    def fill(self, which=("plain", "packed")):
        if "plain" in which:
            self.plain.upload(self.host)
        if "packed" in which:
            self.packed.upload({k: v for k, v in self.host.items() if not k.startswith("tendency_")})
            assert self.hip.hipMemcpy(self.packed.buffer_tmp, self.buf_tmp.ctypes.data, self.buf_tmp.nbytes, 1) == 0
            assert self.hip.hipMemcpy(self.packed.buffer_loc, self.buf_loc.ctypes.data, self.buf_loc.nbytes, 1) == 0

    def scratch(self, variant):
        if variant & 0xff == ca.VARIANT_KSEG and not self.ws.value:
            nbytes = self.lib.cloudsc_gpu_scratch_bytes(self.precision, ca.VARIANT_KSEG, self.ngptot, self.nproma,
                                                        self.ds.klev)
            assert nbytes > 0
            assert self.hip.hipMalloc(C.byref(self.ws), C.c_size_t(nbytes)) == 0
            assert self.hip.hipMemset(self.ws, 0, C.c_size_t(256)) == 0
        return self.ws

    def run_both(self, variant, stream=None, which=("plain", "packed")):
        """cloudsc_gpu_run on `plain`, cloudsc_gpu_run_tendbuf on `packed` (each followed by its check)."""
        ws = self.scratch(variant)
        k = self.ds.klev
        if "plain" in which:
            ca.check(self.lib.cloudsc_gpu_run(0, stream, self.precision, variant, self.ngptot, self.nproma, k,
                                              C.byref(self.plain.f), ws))
            assert self.lib.cloudsc_gpu_check(0, stream, variant & 0xff, ws) == 0
        if "packed" in which:
            ca.gpu_run_tendbuf(self.packed.f, self.precision, variant, self.ngptot, self.nproma, k, self.tend_planes,
                               scratch=ws, stream=stream)
            assert self.lib.cloudsc_gpu_check(0, stream, variant & 0xff, ws) == 0

    def device_mismatches(self, stream=None):
        """Unpack BUFFER_LOC into the packed set's separate arrays, then cloudsc_fields_compare of its 21
        outputs against the plain set's: {member: mismatches} where not 0."""
        loc_src = ca.fields_subset(self.packed.f, tb.LOC)
        loc_dst = ca.fields_subset(self.packed.separate, tb.LOC)
        ca.convert_fields_tendbuf(loc_src, loc_dst, self.ngptot, self.ds.klev, self.precision, self.nproma,
                                  self.tend_planes, self.precision, self.nproma, 0, stream=stream)
        a = ca.fields_subset(self.packed.separate, NAMES)
        b = ca.fields_subset(self.plain.f, NAMES)
        d = ca.compare_fields(a, b, self.ngptot, self.ds.klev, self.precision, self.nproma, self.precision,
                              self.nproma, stream=stream)
        assert sorted(d) == sorted(NAMES)
        assert all(v["compared"] > 0 for v in d.values())
        return {k: v["mismatches"] for k, v in d.items() if v["mismatches"]}

    def host_check(self):
        """The same on the host, and the sentinels: returns the list of what is wrong."""
        self.hip.hipDeviceSynchronize()
        loc = np.empty_like(self.buf_loc)
        tmp = np.empty_like(self.buf_tmp)
        assert self.hip.hipMemcpy(loc.ctypes.data, self.packed.buffer_loc, loc.nbytes, 2) == 0
        assert self.hip.hipMemcpy(tmp.ctypes.data, self.packed.buffer_tmp, tmp.nbytes, 2) == 0
        wrong = []
        if not np.array_equal(tb.bits(tmp), tb.bits(self.buf_tmp)):
            wrong.append("BUFFER_TMP changed")
        if not tb.is_sentinel(loc, tb.untouched_mask(loc, self.lay, tb.LOC, self.ngptot), tb.SENTINEL_LOC):
            wrong.append("BUFFER_LOC: an unbound plane or a padding lane was written")
        for k in NAMES:
            ref = self.plain.download_raw(k)
            if k in tb.LOC:
                got = tb.take(loc, self.lay[k], k)
            else:
                got = self.packed.download_raw(k)
                if not np.array_equal(tb.bits(got), tb.bits(ref)):    # whole arrays: padding lanes included
                    wrong.append("%s: differs (padding included)" % k)
            if not np.array_equal(tb.bits(tc.columns(got, self.ngptot)), tb.bits(tc.columns(ref, self.ngptot))):
                wrong.append("%s: differs" % k)
        return wrong

    def close(self):
        if self.ws.value:
            self.hip.hipFree(self.ws)
            self.ws = C.c_void_p()
        self.plain.close()
        self.packed.close()


CASES = [(n, p, v) for (n, p) in tb.SHAPES for v in VARIANTS if not (p > 256 and v == "kcache")]


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
def validation_table(out):
    lines = out.splitlines()
    start = [i for i, ln in enumerate(lines) if "Variable" in ln and "MaxRelErr" in ln][0]
    return lines[start:]


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
class DeviceSide:
    """A tc.Side mirrored on the device: plain hipMalloc copies of every array and buffer, the Fields
    pointing at the same places in them."""

    def __init__(self, hip, side):
        self.hip, self.side, self.f = hip, side, ca.Fields()
        self.host = list(side.arrays.values()) + (side.bufs or [])
        self.dev = []
        for a in self.host:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
            assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
            self.dev.append(p.value)
        for name, _ in ca.Fields._fields_:
            hp = getattr(side.f, name)
            if hp:
                setattr(self.f, name, self.translate(hp))

    def translate(self, host_ptr):
        for a, d in zip(self.host, self.dev):
            if a.ctypes.data <= host_ptr < a.ctypes.data + a.nbytes:
                return d + (host_ptr - a.ctypes.data)
        raise AssertionError("pointer outside every array")

    def snapshot(self):
        self.hip.hipDeviceSynchronize()
        out = []
        for a, d in zip(self.host, self.dev):
            b = np.empty_like(a)
            assert self.hip.hipMemcpy(b.ctypes.data, d, b.nbytes, 2) == 0
            out.append(b)
        return out

    def close(self):
        for d in self.dev:
            self.hip.hipFree(d)


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
