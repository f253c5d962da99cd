"""The cumulative tendency buffer on the device: cloudsc_gpu_run_tendbuf_cml against the device's own
cloudsc_gpu_run_tendbuf local tendencies plus a host add (raw bits in fp64 and fp32, the widened-input
identity in mixed), against the host form (fp64) and against the prognostic step followed by
cloudsc_fields_accumulate_tendbuf; KCACHE and KSEG (also with forced hand-offs), PROGNOSTIC and SURFACE,
aerosols, packed narrow blocks; the bytes that must not change; one KSEG workspace for every form; two
launches; the CLI's --fields tendbuf-cml and the Python helper."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import form_state_cases as fs
import host_harness as hh
import tendbuf_cases as tb
import tendbuf_cml_cases as cm
from gpu_harness import DIAG, PATTERN, PRECISIONS, Pair, VARIANTS, columns, raw_bits, validation_table
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PROG, SURF, ALL = ca.OUTPUTS_PROGNOSTIC, ca.OUTPUTS_SURFACE, ca.OUTPUTS_ALL
KEPT_OTHER = hh.KEPT_OTHER
CANARY = hh.CANARY


class CmlPair(Pair):
    """Pair whose packed set also has a third device buffer, BUFFER_CML.  Only the packed set is used:
    cloudsc_gpu_run_tendbuf on it gives the device's local tendencies, the fused form runs on the same
    inputs."""

    def __init__(self, lib, hip, ds, ngptot, nproma, precision, tend_planes, order, seed=1, host=None):
        super().__init__(lib, hip, ds, ngptot, nproma, precision, tend_planes, order)
        if host is not None:           # other input values (the widened float state)
            self.host = host
            for n in tb.TMP:
                tb.put(self.buf_tmp, self.lay[n], self.host[n], ngptot)
        self.buf_loc.view(np.uint8)[...] = CANARY
        self.clay = cm.layout(order, tend_planes)
        self.cml0 = cm.make_buffer(self.nb, tend_planes, ds.klev, nproma, self.dt, self.clay, ngptot, seed)
        self.dev_cml = C.c_void_p(self.device_array(np.empty_like(self.cml0)))
        plane = ds.klev * nproma * self.cml0.itemsize
        self.cml = ca.TendCml(*[self.dev_cml.value + self.clay[k] * plane for k in cm.CML])
        self.surf = {}

    def put_cml(self, host_buf=None):
        b = self.cml0 if host_buf is None else host_buf
        assert self.hip.hipMemcpy(self.dev_cml, b.ctypes.data, b.nbytes, 1) == 0

    def device_loc(self, variant):
        """{tendency_loc_*: block-layout array} and the other kept outputs of cloudsc_gpu_run_tendbuf."""
        self.fill(("packed",))
        self.run_both(variant, which=("packed",))
        loc = self.read(self.packed.buffer_loc, self.buf_loc)
        out = {n: tb.take(loc, self.lay[n], n) for n in tb.LOC}
        out.update({n: self.packed.download_raw(n) for n in KEPT_OTHER})
        return out

    def fused_fields(self, outputs, loc):
        f = ca.Fields()
        C.memmove(C.byref(f), C.byref(self.packed.f), C.sizeof(ca.Fields))
        for n in DIAG:
            setattr(f, n, None)
        if loc == "null":
            for n in tb.LOC:
                setattr(f, n, None)
        if outputs == SURF:
            for n in ca.SURFACE_FLUX_FIELDS:
                small = np.empty((self.nb, self.nproma), dtype=self.dt)
                if n not in self.surf:
                    self.surf[n] = self.device_array(small)
                assert self.hip.hipMemset(self.surf[n], PATTERN, C.c_size_t(small.nbytes)) == 0
                setattr(f, n, self.surf[n])
        return f

    def run_fused(self, variant, outputs=PROG, loc="null", refill=True):
        if refill:                      # plude is INOUT; BUFFER_LOC gets its canary back
            self.fill(("packed",))
        f = self.fused_fields(outputs, loc)
        self.checked_step(f, variant, outputs, self.tend_planes, cml=self.cml)
        return self.read(self.dev_cml, self.cml0)

    def check_untouched(self, after, before, ref, outputs):
        """What does not depend on the sums; returns the list of what is wrong."""
        wrong = []
        keep = ~cm.touched_mask(before.shape, self.clay, self.ngptot)
        if not np.array_equal(tb.bits(after)[keep], tb.bits(before)[keep]):
            wrong.append("BUFFER_CML: the vapour plane, an unbound plane or a padding lane changed")
        if not (raw_bits(self.read(self.packed.buffer_loc, self.buf_loc)) == CANARY).all():
            wrong.append("BUFFER_LOC was written")
        if not cm.same_bits(self.read(self.packed.buffer_tmp, self.buf_tmp), self.buf_tmp):
            wrong.append("BUFFER_TMP changed")
        for n in DIAG:
            if not (raw_bits(self.packed.download_raw(n)) == PATTERN).all():
                wrong.append("%s: a diagnostic member was written" % n)
        for n in KEPT_OTHER:
            if outputs == SURF and n in ca.SURFACE_FLUX_FIELDS:
                got = self.read(self.surf[n], np.empty((self.nb, self.nproma), dtype=self.cml0.dtype))
                want = ref[n][:, self.ds.klev, :]
                if not cm.same_bits(columns(got, self.ngptot), columns(want, self.ngptot)):
                    wrong.append("%s: the surface row differs" % n)
                tail = self.ngptot - (self.nb - 1) * self.nproma
                if not (raw_bits(got[self.nb - 1, tail:]) == PATTERN).all():
                    wrong.append("%s: a padding lane was written" % n)
                if not (raw_bits(self.packed.download_raw(n)) == PATTERN).all():
                    wrong.append("%s: the profile was written" % n)
            elif not cm.same_bits(self.packed.download_raw(n), ref[n]):
                wrong.append("%s: differs" % n)
        return wrong


# (ngptot, nproma, variant, planes, order, outputs, loc, pack mode)
CASES = [
    (300, 64, "kseg", 11, "permuted", PROG, "canary", -1),
    (300, 64, "kcache", 8, "reference", SURF, "null", -1),
    (200, 128, "kseg", 8, "reference", SURF, "canary", -1),     # two sub-blocks per block
    (100, 16, "kseg", 11, "permuted", SURF, "null", -1),        # packed narrow blocks (the default)
    (100, 16, "kcache", 11, "permuted", PROG, "canary", -1),
    (100, 5, "kseg", 8, "reference", PROG, "canary", 1),        # NPROMA 5 packed ...
    (100, 5, "kseg", 11, "permuted", PROG, "null", 0),          # ... and unpacked
    (100, 5, "kcache", 11, "permuted", SURF, "canary", 1),
]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("ngptot,nproma,variant,planes,order,outputs,loc,pack", CASES)
def test_fused_is_device_loc_plus_host_add(lib, hip, ds, ngptot, nproma, variant, planes, order, outputs, loc, pack,
                                           precision):
    prec = PRECISIONS[precision]
    pr = CmlPair(lib, hip, ds, ngptot, nproma, prec, planes, order, seed=ngptot + nproma)
    try:
        ca.narrow_pack(pack)
        ref = pr.device_loc(VARIANTS[variant])
        pr.put_cml()
        after = pr.run_fused(VARIANTS[variant], outputs, loc)
        assert pr.check_untouched(after, pr.cml0, ref, outputs) == []
        assert cm.same_bits(after, cm.expected(pr.cml0, pr.clay, ngptot, ref, cm.add_storage))
        if prec == ca.FP64:             # and the host form on the same buffer
            st, f, buf_tmp, buf_loc = hh.host_set(ds, ngptot, nproma, prec, planes, order, outputs, "null")
            host = pr.cml0.copy()
            ca.cpu_run_tendbuf_cml(ca.Params.from_dict(ds.params), f, cm.bind(pr.clay, host), prec, outputs, ngptot,
                                   nproma, ds.klev, planes, nthreads=4)
            assert cm.same_bits(after, host)
    finally:
        pr.close()


@pytest.mark.parametrize("name,nproma,variant", [("W", 64, "kseg"), ("M", 16, "kcache"), ("klev3", 64, "kseg"),
                                                 ("klev274", 64, "kseg"), ("aerosol_W", 64, "kseg"),
                                                 ("aerosol_W", 16, "kcache")])
def test_fused_fp64_on_state(lib, hip, ds, scenarios, name, nproma, variant):
    s = fs.dataset(name, ds, scenarios)
    n = fs.NGPTOT
    pr = CmlPair(lib, hip, s, n, nproma, ca.FP64, 11, "permuted", seed=5)
    try:
        assert pr.aer == (name == "aerosol_W")
        ref = pr.device_loc(VARIANTS[variant])
        pr.put_cml()
        after = pr.run_fused(VARIANTS[variant], PROG, "null")
        assert pr.check_untouched(after, pr.cml0, ref, PROG) == []
        assert cm.same_bits(after, cm.expected(pr.cml0, pr.clay, n, ref, cm.add_storage))
        if fs.rain_active(name):
            d = after[:, pr.clay["cld"] + cm.QR] != pr.cml0[:, pr.clay["cld"] + cm.QR]
            assert np.count_nonzero(d) > 0          # the rain tendency reached its cumulative plane
    finally:
        pr.close()


@pytest.mark.parametrize("ngptot,nproma,variant,outputs", [(300, 64, "kseg", PROG), (100, 16, "kcache", SURF),
                                                           (100, 5, "kseg", PROG)])
def test_fused_mixed_identity(lib, hip, ds, ngptot, nproma, variant, outputs):
    """out = (float) fp64_form((double) in), CML included: the mixed launch on float buffers against the fp64
    launch on the same values widened."""
    planes, order = 11, "permuted"
    p32 = CmlPair(lib, hip, ds, ngptot, nproma, ca.MIXED, planes, order, seed=9)
    wide = {k: (a if a.dtype == np.int32 else a.astype(np.float64)) for k, a in p32.host.items()}
    p64 = CmlPair(lib, hip, ds, ngptot, nproma, ca.FP64, planes, order, seed=9, host=wide)
    try:
        ref32 = p32.device_loc(VARIANTS[variant])
        p32.put_cml()
        after32 = p32.run_fused(VARIANTS[variant], outputs, "canary")
        assert p32.check_untouched(after32, p32.cml0, ref32, outputs) == []
        m = cm.touched_mask(p32.cml0.shape, p32.clay, ngptot)
        start64 = np.zeros(p32.cml0.shape, dtype=np.float64)
        start64[m] = p32.cml0[m].astype(np.float64)
        p64.put_cml(start64)
        after64 = p64.run_fused(VARIANTS[variant], outputs, "null")
        assert np.array_equal(tb.bits(after32)[m], tb.bits(after64.astype(np.float32))[m])
        # not the separate pass's rule: adding the narrowed float differs somewhere
        assert not cm.same_bits(after32, cm.expected(p32.cml0, p32.clay, ngptot, ref32, cm.add_storage))
    finally:
        p32.close()
        p64.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32", "mixed"])
@pytest.mark.parametrize("lpl,cpl", [(11, 11), (0, 11), (11, 0)])
def test_device_pass_and_fused_is_step_plus_pass(lib, hip, ds, precision, lpl, cpl):
    """cloudsc_fields_accumulate_tendbuf against NumPy on whole buffers; with both sides packed (fp64, fp32),
    the fused form equals the prognostic step followed by the pass."""
    prec, ngptot, nproma, planes = PRECISIONS[precision], 300, 64, 11
    pr = CmlPair(lib, hip, ds, ngptot, nproma, prec, planes, "permuted", seed=13)
    extra = []
    try:
        ref = pr.device_loc(ca.VARIANT_KSEG)                       # BUFFER_LOC now holds the step's tendencies
        loc_before = pr.read(pr.packed.buffer_loc, pr.buf_loc)
        pr.put_cml()
        loc = ca.fields_subset(pr.packed.f, tb.LOC)
        dt = pr.cml0.dtype
        if not lpl:                                                # the tendencies in separate arrays
            for n in tb.LOC:
                a = np.ascontiguousarray(ref[n])
                p = C.c_void_p()
                assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
                extra.append(p)
                assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
                setattr(loc, n, p.value)
        if cpl:
            ca.accumulate_tendbuf(loc, pr.cml, prec, ngptot, nproma, ds.klev, lpl, cpl)
            got = pr.read(pr.dev_cml, pr.cml0)
            want = cm.expected(pr.cml0, pr.clay, ngptot, ref, cm.add_storage)
            assert cm.same_bits(got, want)
            assert cm.same_bits(pr.read(pr.packed.buffer_loc, pr.buf_loc), loc_before)      # the source is only read
            if lpl and prec != ca.MIXED:
                pr.put_cml()
                fused = pr.run_fused(ca.VARIANT_KSEG, PROG, "null")
                assert cm.same_bits(fused, got)
        else:                                                      # the cumulative planes as separate arrays
            c, hosts = ca.TendCml(), []
            for k in cm.CML:
                n = ca.NCLV if k == "cld" else 1
                h = cm.make_buffer(pr.nb, n, ds.klev, nproma, dt, {j: (0 if j == k else 99) for j in cm.CML}, ngptot, 17)
                p = C.c_void_p()
                assert hip.hipMalloc(C.byref(p), C.c_size_t(h.nbytes)) == 0
                extra.append(p)
                assert hip.hipMemcpy(p, h.ctypes.data, h.nbytes, 1) == 0
                setattr(c, k, p.value)
                hosts.append((k, h, p))
            ca.accumulate_tendbuf(loc, c, prec, ngptot, nproma, ds.klev, lpl, 0)
            for k, h, p in hosts:
                want = cm.expected(h, {j: (0 if j == k else 99) for j in cm.CML}, ngptot, ref, cm.add_storage)
                assert cm.same_bits(pr.read(p, h), want), k
            assert cm.same_bits(pr.read(pr.packed.buffer_loc, pr.buf_loc), loc_before)
    finally:
        for p in extra:
            hip.hipFree(p)
        pr.close()


def test_kseg_forced_handoffs_and_two_launches(lib, hip, ds):
    pr = CmlPair(lib, hip, ds, 300, 64, ca.FP64, 8, "reference", seed=3)
    try:
        ref = pr.device_loc(ca.VARIANT_KSEG)
        pr.put_cml()
        ca.kseg_schedule(3, 3)                                      # three segments on three workgroups
        once = pr.run_fused(ca.VARIANT_KSEG, PROG, "canary")
        exp1 = cm.expected(pr.cml0, pr.clay, 300, ref, cm.add_storage)
        assert cm.same_bits(once, exp1)
        twice = pr.run_fused(ca.VARIANT_KSEG, PROG, "canary")       # a launch adds once: the second adds again
        assert cm.same_bits(twice, cm.expected(exp1, pr.clay, 300, ref, cm.add_storage))
        assert pr.check_untouched(twice, pr.cml0, ref, PROG) == []
    finally:
        pr.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_one_kseg_workspace_for_every_form(lib, hip, ds, precision):
    prec = PRECISIONS[precision]
    pr = CmlPair(lib, hip, ds, 300, 64, prec, 11, "permuted", seed=4)
    try:
        ref = pr.device_loc(ca.VARIANT_KSEG)                        # ALL (cloudsc_gpu_run_tendbuf) on the workspace
        exp = cm.expected(pr.cml0, pr.clay, 300, ref, cm.add_storage)
        ws = pr.scratch(ca.VARIANT_KSEG)
        for outputs in (PROG, SURF):
            f = pr.fused_fields(outputs, "canary")                  # the step of that selection, then the fused form
            pr.fill(("packed",))
            ca.gpu_run_tendbuf_outputs(f, prec, ca.VARIANT_KSEG, outputs, 300, 64, ds.klev, 11, scratch=ws)
            assert lib.cloudsc_gpu_check(0, None, ca.VARIANT_KSEG, ws) == 0
            pr.put_cml()
            assert cm.same_bits(pr.run_fused(ca.VARIANT_KSEG, outputs, "canary"), exp), outputs
        again = pr.device_loc(ca.VARIANT_KSEG)                      # and ALL again
        assert all(cm.same_bits(again[n], ref[n]) for n in ref)
    finally:
        pr.close()


def test_python_helper_round_trip(lib, hip, ds):
    """bind_tendbuf_three on device buffers in the reference's order, no BUFFER_LOC: the fused launch through
    the returned pair."""
    pr = CmlPair(lib, hip, ds, 100, 16, ca.FP64, 8, "reference", seed=6)
    try:
        ref = pr.device_loc(ca.VARIANT_KCACHE)
        pr.put_cml()
        pr.fill(("packed",))
        f = pr.fused_fields(PROG, "canary")
        f, c = ca.bind_tendbuf_three(f, ca.FP64, 16, ds.klev, pr.packed.buffer_tmp, pr.dev_cml.value)
        assert f.tendency_loc_t is None and (c.t, c.q, c.a, c.cld) == (pr.cml.t, pr.cml.q, pr.cml.a, pr.cml.cld)
        ca.gpu_run_tendbuf_cml(f, c, ca.FP64, ca.VARIANT_KCACHE, PROG, 100, 16, ds.klev, 8)
        assert cm.same_bits(pr.read(pr.dev_cml, pr.cml0), cm.expected(pr.cml0, pr.clay, 100, ref, cm.add_storage))
    finally:
        pr.close()


@pytest.mark.parametrize("outputs", ["prognostic", "surface"])
def test_cli_tendbuf_cml_prints_the_inplace_rows(outputs):
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    base = [exe, "1", "300", "64", "--reps", "2", "--warmup", "1", "--tend-planes", "11", "--outputs", outputs]
    got = subprocess.run(base + ["--fields", "tendbuf-cml"], capture_output=True, text=True, timeout=120)
    want = subprocess.run(base + ["--fields", "tendbuf-inplace"], capture_output=True, text=True, timeout=120)
    assert got.returncode == 0 and want.returncode == 0, got.stderr + want.stderr
    a, b = validation_table(got.stdout), validation_table(want.stdout)
    assert a == b                                   # 0 + loc: the rows of BUFFER_LOC validated in place
    assert len([ln for ln in a if "TENDENCY_LOC" in ln]) == 4 and len(a) == 1 + 11 + 1
    assert "VALIDATION: PASSED" in a[-1]
