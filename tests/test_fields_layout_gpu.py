"""Layout conversion on the device (cloudsc_fields_convert_layout): the shapes of tests/test_fields_layout_cpu.py
compared on raw bits with the host form (itself held to the NumPy restatement there), and the physics run
from and into level-contiguous [ngptot][rows] arrays against the unchanged state API."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import fields_convert_cases as fc
import fields_layout_cases as lc
import mixed_expected as mx
from gpu_harness import lib, hip, run_on  # noqa: F401  (lib, hip: fixtures)

pytestmark = pytest.mark.gpu

B, L = lc.B, lc.L
VALIDATED = [k for _, k in ca.VALIDATED]


def cpu_expected(lib, src, dst_layout, dnp, dp, names=None):
    """The host form's result on the same host arrays: a sentinel-filled HostSet after the conversion."""
    dst = src.like(dst_layout, nproma=dnp, precision=dp)
    ca.check(lib.cloudsc_cpu_fields_convert_layout(2, src.ngptot, src.klev, src.outputs, src.precision, src.layout,
                                                   src.nproma, C.byref(src.fields(names)), dp, dst.layout, dst.nproma,
                                                   C.byref(dst.fields(names))))
    return dst


class Arena:
    """The arrays of a HostSet in one device buffer, each followed by a guard margin, uploaded as they are
    (a destination: all sentinel)."""

    def __init__(self, hip, hs):
        self.hip, self.hs, self.offs, self.p = hip, hs, {}, C.c_void_p()
        total = 0
        for n in hs.names:
            self.offs[n] = total
            total += (hs.full[n].nbytes + 255) // 256 * 256
        self.total = total
        self.host = np.full(total, fc.SENTINEL_BYTE, dtype=np.uint8)
        for n in hs.names:
            self.host[self.offs[n]:self.offs[n] + hs.full[n].nbytes] = hs.full[n].view(np.uint8)
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(total)) == 0
        assert hip.hipMemcpy(self.p, self.host.ctypes.data, C.c_size_t(total), 1) == 0

    def fields(self, names=None):
        f = ca.Fields()
        for n in (self.hs.names if names is None else names):
            setattr(f, n, self.p.value + self.offs[n])
        return f

    def download(self):
        assert self.hip.hipDeviceSynchronize() == 0
        got = np.empty(self.total, dtype=np.uint8)
        assert self.hip.hipMemcpy(got.ctypes.data, self.p, C.c_size_t(self.total), 2) == 0
        return got

    def close(self):
        if self.p.value:
            self.hip.hipFree(self.p)
            self.p = C.c_void_p()


def device_convert(hip, src, exp, names=None, stream=None):
    """src -> a sentinel-filled device image of exp's shape; returns the image and what it has to be: exp's
    buffers (padding lanes and guard margins still the sentinel) and sentinel everywhere else."""
    a, b = Arena(hip, src), Arena(hip, exp.like())
    try:
        ca.convert_fields_layout(a.fields(names), b.fields(names), src.ngptot, src.klev, src.precision, src.layout,
                                 src.nproma, exp.precision, exp.layout, exp.nproma, src.outputs, 0, stream)
        if stream is not None:
            assert hip.hipStreamSynchronize(stream) == 0
        got = b.download()
        want = np.full(b.total, fc.SENTINEL_BYTE, dtype=np.uint8)
        for n in exp.names:
            want[b.offs[n]:b.offs[n] + exp.full[n].nbytes] = exp.full[n].view(np.uint8)
        return got, want
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------
# the device form against the host form: shapes, storage pairs, ktype, padding lanes and guard margins
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,storage", lc.CASES, ids=lc.CASE_IDS)
def test_device_matches_cpu_form(lib, hip, shape, storage):
    (ngptot, nproma, klev), (sp, dp) = shape, storage
    for src in (lc.HostSet(B, ngptot, nproma, klev, sp).fill_random(1), lc.HostSet(L, ngptot, 0, klev, sp).fill_random(2)):
        exp = cpu_expected(lib, src, L if src.layout == B else B, nproma, dp)
        got, want = device_convert(hip, src, exp)
        assert np.array_equal(got, want), "b2l" if src.layout == B else "l2b"


@pytest.mark.parametrize("sl,dl", [(L, L), (B, B)], ids=["l2l", "b2b"])
def test_same_layout_forwards(lib, hip, sl, dl):
    src = lc.HostSet(sl, 300, 0 if sl == L else 24, 17, ca.FP64).fill_random()
    exp = cpu_expected(lib, src, dl, 64, ca.MIXED)
    got, want = device_convert(hip, src, exp)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("names", [lc.INPUTS, lc.OUTPUTS], ids=["inputs", "outputs"])
def test_device_subset(lib, hip, names):
    src = lc.HostSet(L, 300, 0, 17, ca.FP64).fill_random()
    exp = cpu_expected(lib, src, B, 64, ca.MIXED, names=names)
    got, want = device_convert(hip, src, exp, names=names)      # every other member still the sentinel
    assert np.array_equal(got, want)


@pytest.mark.parametrize("sl,dl", [(B, L), (L, B)], ids=["b2l", "l2b"])
def test_device_outputs_surface(lib, hip, sl, dl):
    names = list(ca.SURFACE_FLUX_FIELDS) + ["pcovptot", "tendency_loc_cld", "plude"]
    src = lc.HostSet(sl, 300, 0 if sl == L else 24, 17, ca.FP64, names, ca.OUTPUTS_SURFACE).fill_random()
    exp = cpu_expected(lib, src, dl, 64, ca.FP64)
    got, want = device_convert(hip, src, exp)
    assert np.array_equal(got, want)


def test_non_default_stream(lib, hip):
    st = C.c_void_p()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipStreamCreateWithFlags(C.byref(st), C.c_uint(1)) == 0      # hipStreamNonBlocking
    try:
        for src in (lc.HostSet(B, 300, 24, 17, ca.FP64).fill_random(), lc.HostSet(L, 300, 0, 17, ca.FP64).fill_random()):
            exp = cpu_expected(lib, src, L if src.layout == B else B, 64, ca.MIXED)
            got, want = device_convert(hip, src, exp, stream=st)
            assert np.array_equal(got, want)
    finally:
        hip.hipStreamDestroy(st)


def test_kernels_use_no_scratch(lib):
    """What the loaded code object says: no scratch, and at most 32 KiB of LDS per workgroup
    (profiles/fields_layout/kernel_resources.txt is the compiler's record)."""
    lib.cloudsc_debug_layout_kernel_resources.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    for which in range(8):
        scratch, lds = C.c_int(-1), C.c_int(-1)
        ca.check(lib.cloudsc_debug_layout_kernel_resources(0, which, C.byref(scratch), C.byref(lds)))
        assert scratch.value == 0 and 0 < lds.value <= 32768, (which, scratch.value, lds.value)


# ---------------------------------------------------------------------------
# the physics through level-contiguous arrays
# ---------------------------------------------------------------------------
def levels_inputs(ds, n):
    """The dataset's inputs at n columns as [ngptot][rows] / [ngptot] float64 (int32 ktype) arrays."""
    host = ca.make_host_state(ds, n, n, ca.FP64)
    return {k: np.ascontiguousarray(host.arrays[k].reshape(-1, n).T) for k in lc.INPUTS}


def through_levels(lib, hip, ds, n, precision, variant):
    """LEVELS doubles -> a placed NPROMA 64 set of `precision` -> one step -> the outputs as LEVELS arrays."""
    lev = ca.DeviceFields(n, 0, ds.klev, ca.FP64, layout=L)
    df = ca.DeviceFields(n, 64, ds.klev, precision)
    out = ca.DeviceFields(n, 0, ds.klev, precision, layout=L)
    try:
        assert lev.shape("pt") == (n, ds.klev) and lev.shape("pclv") == (n, 5 * ds.klev) and lev.shape("plsm") == (n,)
        assert lev.nbytes("paph") == n * (ds.klev + 1) * 8 and out.nbytes("ktype") == n * 4
        lev.upload({k: (a[:, 0] if lev.shape(k) == (n,) else a) for k, a in levels_inputs(ds, n).items()})
        lev.convert_to(df, names=lc.INPUTS)
        run_on(lib, hip, ds, df, variant)
        df.convert_to(out, names=VALIDATED)
        got = {k: out.download_raw(k) for k in VALIDATED}
        assert all(got[k].shape == out.shape(k) for k in VALIDATED)
        return got
    finally:
        lev.close()
        df.close()
        out.close()


@pytest.mark.parametrize("variant", [ca.VARIANT_KSEG, ca.VARIANT_KCACHE], ids=["kseg", "kcache"])
def test_physics_through_levels_fp64(lib, hip, ds, variant):
    """The state API's outputs, transposed on the host, bit for bit."""
    n = 300
    got = through_levels(lib, hip, ds, n, ca.FP64, variant)
    g = ca.GpuState(ds, n, 64, ca.FP64)
    try:
        g.run(variant, 1)
        want = g.outputs()
    finally:
        g.close()
    for k in VALIDATED:
        w = np.ascontiguousarray(want[k].reshape(-1, n).T).reshape(got[k].shape)
        assert got[k].dtype == np.float64 and np.array_equal(fc.bits(got[k]), fc.bits(w)), k


def test_physics_through_levels_mixed(lib, hip, ds):
    """CLOUDSC_MIXED from LEVELS doubles: the bits of a mixed state made from the same doubles."""
    n = 300
    got = through_levels(lib, hip, ds, n, ca.MIXED, ca.VARIANT_KSEG)
    gm = ca.GpuState(ds, n, 64, ca.MIXED)
    try:
        gm.run(ca.VARIANT_KSEG, 1)
        want = {k: mx.as_f32(v) for k, v in gm.outputs().items()}
    finally:
        gm.close()
    got = {k: np.ascontiguousarray(a.reshape(n, -1).T).reshape(want[k].shape) for k, a in got.items()}
    assert mx.mismatches(got, want) == {}


def test_python_refuses_steps_on_a_levels_set(lib):
    lev = ca.DeviceFields(64, 0, 3, ca.FP64, layout=L)
    try:
        with pytest.raises(ValueError, match="LAYOUT_LEVELS"):
            ca.gpu_run_outputs(lev.f, ca.FP64, ca.VARIANT_KCACHE, ca.OUTPUTS_ALL, 64, 64, 3)
        with pytest.raises(ValueError, match="LAYOUT_LEVELS"):
            lev.compare(lev)
    finally:
        lev.close()
    with pytest.raises(ValueError):
        ca.DeviceFields(64, 64, 3, ca.FP64, layout=L)


# ---------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------
def run_cli(*args):
    exe = os.path.join(ca.HERE, "dwarf-cloudsc-amd")
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_cli_fields_levels(precision):
    """--fields levels prints --fields caller's tables: the same validation rows."""
    rows = {}
    for mode in ("caller", "levels"):
        r = run_cli(1, 300, 64, "--fields", mode, "--precision", precision)
        assert r.returncode == 0, r.stdout + r.stderr
        rows[mode] = [ln for ln in r.stdout.splitlines() if "D1 " in ln or "D2 " in ln or "D3 " in ln]
        assert len(rows[mode]) == 21, r.stdout
    assert rows["levels"] == rows["caller"]


@pytest.mark.parametrize("variant", ["cpu", "scc", "scc-private"])
def test_cli_fields_levels_refuses_other_variants(variant):
    r = run_cli(1, 300, 64, "--fields", "levels", "--variant", variant)
    assert r.returncode != 0 and "levels" in (r.stdout + r.stderr)
