"""Per-column parameter multipliers (SPP) on the device: cloudsc_gpu_run_spp with all-ones fields against
cloudsc_gpu_run_outputs on raw bits (KCACHE and KSEG, three precisions, ALL and PROGNOSTIC, packed and unpacked
narrow blocks); with tuples that vary by column against the oracle (fp64) and against the device's own ordinary
step under each tuple's host-scaled parameter set; KSEG with forced hand-offs and other KLEV; the bytes that must
not change; one KSEG workspace for both forms; the argument rules; the CLI's --spp unit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import form_state_cases as fs
import spp_cases as sp
import test_outputs_gpu as og
import test_spp_cpu as tsc

pytestmark = pytest.mark.gpu

ALL, PROG = ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC
NAMES = fs.NAMES
DIAG, KEPT = og.DIAG, og.KEPT
PRECISIONS, VARIANTS = og.PRECISIONS, og.VARIANTS
PATTERN = og.PATTERN


@pytest.fixture(scope="module")
def lib():
    lib = ca.gpu_lib()
    assert ca.device_count() > 0
    return lib


@pytest.fixture(scope="module")
def hip():
    h = ca._hip()
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    return h


@pytest.fixture(autouse=True)
def restore_knobs():
    yield
    ca.narrow_pack(-1)
    ca.kseg_schedule(0, 0)


def columns(blocks, ngptot):
    return np.ascontiguousarray(ca.blocks_to_columns(blocks, ngptot))


class Dev:
    """One problem on the device: a field set with all 21 outputs allocated and pattern-filled, the five
    multiplier fields, the KSEG workspace; the device's default parameter set is the state's."""

    def __init__(self, lib, hip, s, ngptot, nproma, precision, mult):
        self.lib, self.hip, self.s = lib, hip, s
        self.ngptot, self.nproma, self.precision = ngptot, nproma, precision
        self.aer = fs.uses_aerosols(s)
        self.host = og.host_inputs(s, ngptot, nproma, precision)
        self.df = ca.DeviceFields(ngptot, nproma, s.klev, precision, place=False, aerosols=self.aer)
        self.ws = C.c_void_p()
        self.mult, self.dmult = mult, {}
        for k, a in mult.items():
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
            assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
            self.dmult[k] = p
        self.spp = ca.Spp(*[self.dmult[k].value if k in self.dmult else None for k in sp.SLOTS])
        self.init_params(s.params)

    def init_params(self, params):
        p = ca.Params.from_dict(params)
        ca.check(self.lib.cloudsc_gpu_init(0, C.byref(p)))

    def scratch(self, variant):
        if variant == ca.VARIANT_KSEG and not self.ws.value:
            n = self.lib.cloudsc_gpu_scratch_bytes(self.precision, variant, self.ngptot, self.nproma, self.s.klev)
            assert n > 0 and self.hip.hipMalloc(C.byref(self.ws), C.c_size_t(n)) == 0
            assert self.hip.hipMemset(self.ws, 0, C.c_size_t(256)) == 0
        return self.ws

    def step(self, variant, outputs, spp):
        """One step on freshly uploaded inputs and pattern-filled outputs; {name: block-layout array}."""
        self.df.upload(self.host)
        ws = self.scratch(variant)
        k = self.s.klev
        if spp:
            ca.gpu_run_spp(self.df.f, self.spp, self.precision, variant, outputs, self.ngptot, self.nproma, k, scratch=ws)
        else:
            ca.gpu_run_outputs(self.df.f, self.precision, variant, outputs, self.ngptot, self.nproma, k, scratch=ws)
        assert self.lib.cloudsc_gpu_check(0, None, variant, ws) == 0
        return {n: self.df.download_raw(n) for n in NAMES}

    def plain_per_tuple(self, variant, outputs, names):
        """The device's own ordinary step once per tuple, each under its host-scaled parameter set uploaded as
        the device's default set (and the state's own set put back): [{name: [..][ngptot]}]."""
        per = []
        try:
            for t in sp.TUPLES:
                self.init_params(sp.scaled_params(self.s.params, t, self.precision))
                out = self.step(variant, outputs, spp=False)
                per.append({n: columns(out[n], self.ngptot) for n in names})
        finally:
            self.init_params(self.s.params)
        return per

    def untouched(self, out, outputs):
        """What a step must leave alone; the list of what is wrong."""
        wrong = []
        for k, a in self.mult.items():
            got = np.empty_like(a)
            assert self.hip.hipMemcpy(got.ctypes.data, self.dmult[k], a.nbytes, 2) == 0
            if not np.array_equal(sp.bits(got), sp.bits(a)):
                wrong.append("multiplier %s changed" % k)
        for n in list(ca.INPUT_FIELDS) + (list(ca.AEROSOL_FIELDS) if self.aer else []):
            if n in self.host and getattr(self.df.f, n) and not np.array_equal(sp.bits(self.df.download_raw(n)), sp.bits(self.host[n])):
                wrong.append("input %s changed" % n)
        tail = self.ngptot % self.nproma
        for n in (KEPT if outputs == PROG else NAMES):
            if tail and not (sp.bits(out[n][-1][..., tail:]) == PATTERN).all():
                wrong.append("%s: a padding lane was written" % n)
        if outputs == PROG:
            wrong += ["%s: written by a PROGNOSTIC run" % n for n in DIAG if not (sp.bits(out[n]) == PATTERN).all()]
        return wrong

    def close(self):
        for p in list(self.dmult.values()) + [self.ws]:
            if p.value:
                self.hip.hipFree(p)
        self.dmult, self.ws = {}, C.c_void_p()
        self.df.close()


def same(a, b, names, ngptot):
    return [n for n in names if not np.array_equal(sp.bits(columns(a[n], ngptot)), sp.bits(columns(b[n], ngptot)))]


# ---------------------------------------------------------------------------
# every multiplier 1.0: cloudsc_gpu_run_outputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [ALL, PROG], ids=["all", "prognostic"])
@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("nproma,pack", [(64, -1), (16, 1), (16, 0)], ids=["np64", "np16_packed", "np16_unpacked"])
def test_all_ones_is_run_outputs(lib, hip, ds, scenarios, nproma, pack, variant, precision, outputs):
    s, n, prec, v = fs.dataset("M", ds, scenarios), fs.NGPTOT, PRECISIONS[precision], VARIANTS[variant]
    d = Dev(lib, hip, s, n, nproma, prec, sp.uniform_fields(n, nproma, prec, sp.TUPLES[0]))
    try:
        ca.narrow_pack(pack)
        geo = ca.launch_geometry(prec, v, n, nproma, s.klev)
        assert geo["pack"] == (4 if (nproma, pack) == (16, 1) else 1)
        want = d.step(v, outputs, spp=False)
        got = d.step(v, outputs, spp=True)
        names = KEPT if outputs == PROG else NAMES
        assert [k for k in names if not np.array_equal(sp.bits(got[k]), sp.bits(want[k]))] == []   # padding included
        assert d.untouched(got, outputs) == []
        assert not (sp.bits(got["pfplsn"]) == PATTERN).all()                 # the step did something
    finally:
        d.close()


# ---------------------------------------------------------------------------
# tuples that vary by column
# ---------------------------------------------------------------------------
_oracle = {}


def oracle_expected(oracle_mod, name, s, ngptot):
    if (name, ngptot) not in _oracle:
        def step(x):
            st, _ = oracle_mod.run_oracle(x, ngptot, fs.ORACLE_NPROMA)
            return {k: columns(st.arrays[k], ngptot) for k in NAMES}
        e = sp.expected_mixed_tuples(step, s, ngptot, ca.FP64, NAMES)
        for a in e.values():
            a.setflags(write=False)
        _oracle[(name, ngptot)] = e
    return _oracle[(name, ngptot)]


def mixed_tuples_check(lib, hip, oracle_mod, name, s, ngptot, nproma, variant, prec, outputs=ALL):
    d = Dev(lib, hip, s, ngptot, nproma, prec, sp.multiplier_fields(ngptot, nproma, prec))
    try:
        names = KEPT if outputs == PROG else NAMES
        got = d.step(variant, outputs, spp=True)
        assert d.untouched(got, outputs) == []
        gotc = {k: columns(got[k], ngptot) for k in names}
        if prec == ca.FP64:
            want = oracle_expected(oracle_mod, name, s, ngptot)
            assert [k for k in names if not np.array_equal(sp.bits(gotc[k]), sp.bits(want[k]))] == []
        own = sp.select_columns(d.plain_per_tuple(variant, outputs, names), ngptot, names)
        assert [k for k in names if not np.array_equal(sp.bits(gotc[k]), sp.bits(own[k]))] == []
        plain = d.step(variant, outputs, spp=False)                          # and not the unperturbed step
        return same(got, plain, names, ngptot)
    finally:
        d.close()


CASES = [("M", 100, 64, "kseg"), ("M", 100, 64, "kcache"), ("M", 100, 16, "kseg"), ("M", 100, 16, "kcache"),
         ("M", 200, 128, "kseg"), ("M", 200, 128, "kcache"), ("aerosol_W", 100, 64, "kseg"),
         ("aerosol_W", 100, 16, "kcache"), ("aerosol_W", 200, 128, "kseg")]


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("name,ngptot,nproma,variant", CASES)
def test_mixed_tuples(lib, hip, ds, scenarios, oracle_mod, name, ngptot, nproma, variant, precision):
    s = fs.dataset(name, ds, scenarios)
    differs = mixed_tuples_check(lib, hip, oracle_mod, name, s, ngptot, nproma, VARIANTS[variant], PRECISIONS[precision])
    assert differs != []


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_mixed_tuples_prognostic(lib, hip, ds, scenarios, oracle_mod, precision):
    s = fs.dataset("M", ds, scenarios)
    assert mixed_tuples_check(lib, hip, oracle_mod, "M", s, 100, 64, ca.VARIANT_KSEG, PRECISIONS[precision], PROG) != []


@pytest.mark.parametrize("name,nproma,precision", [("M", 64, "fp64"), ("M", 64, "mixed"), ("M", 16, "fp32"),
                                                   ("klev3", 64, "fp64"), ("klev274", 64, "fp64")])
def test_kseg_forced_handoffs(lib, hip, ds, scenarios, oracle_mod, name, nproma, precision):
    """Three segments on fewer workgroups than items: every column's state crosses the workspace twice, and the
    later segments must form the column's perturbed values again."""
    s = fs.dataset(name, ds, scenarios)
    ca.kseg_schedule(3, 3)
    geo = ca.launch_geometry(PRECISIONS[precision], ca.VARIANT_KSEG, 100, nproma, s.klev)
    assert geo["workgroups"] == 3 and 3 * geo["units"] > 3
    mixed_tuples_check(lib, hip, oracle_mod, name, s, 100, nproma, ca.VARIANT_KSEG, PRECISIONS[precision])


def test_one_kseg_workspace_for_both_forms(lib, hip, ds, scenarios, oracle_mod):
    s = fs.dataset("M", ds, scenarios)
    d = Dev(lib, hip, s, 100, 64, ca.FP64, sp.multiplier_fields(100, 64, ca.FP64))
    try:
        ca.kseg_schedule(3, 0)
        first = d.step(ca.VARIANT_KSEG, ALL, spp=False)          # each step ends with cloudsc_gpu_check == 0
        mid = d.step(ca.VARIANT_KSEG, PROG, spp=True)
        last = d.step(ca.VARIANT_KSEG, ALL, spp=False)
        assert same(first, last, NAMES, 100) == []
        want = oracle_expected(oracle_mod, "M", s, 100)
        assert [k for k in KEPT if not np.array_equal(sp.bits(columns(mid[k], 100)), sp.bits(want[k]))] == []
        plain = tsc.oracle_step(oracle_mod)(s)
        assert [k for k in NAMES if not np.array_equal(sp.bits(columns(first[k], 100)), sp.bits(plain[k]))] == []
    finally:
        d.close()


# ---------------------------------------------------------------------------
# argument rules, the CLI
# ---------------------------------------------------------------------------
def test_argument_rules_on_the_device(lib, hip, ds):
    tsc.test_gpu_run_spp_rules_need_no_gpu(lib)
    d = Dev(lib, hip, ds, 100, 64, ca.FP32, sp.uniform_fields(100, 64, ca.FP32, sp.TUPLES[1]))
    try:
        ws = d.scratch(ca.VARIANT_KSEG)
        before = lib.cloudsc_last_hip_error()

        def run(variant=ca.VARIANT_KSEG, outputs=ALL, spp=d.spp, f=d.df.f):
            return lib.cloudsc_gpu_run_spp(0, None, ca.FP32, variant, outputs, 100, 64, ds.klev, C.byref(f),
                                           C.byref(spp) if spp is not None else None, ws)
        for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM,
                        ca.VARIANT_KCACHE | ca.FP32_EXACT_LIBM):
            assert run(variant=variant) == ca.EINVAL
        assert run(outputs=ca.OUTPUTS_SURFACE) == ca.EINVAL and run(outputs=7) == ca.EINVAL
        assert run(spp=None) == ca.EINVAL and run(spp=ca.Spp()) == ca.EINVAL
        alias = ca.Spp(*[d.spp.ramid] * 5)
        alias.rpecons = d.df.f.plsm
        assert run(spp=alias) == ca.EINVAL
        assert lib.cloudsc_last_hip_error() == before
        assert run() == 0 and lib.cloudsc_gpu_check(0, None, ca.VARIANT_KSEG, ws) == 0
    finally:
        d.close()


@pytest.mark.parametrize("extra", [[], ["--variant", "kcache", "--precision", "mixed", "--outputs", "prognostic"]],
                         ids=["kseg_fp64", "kcache_mixed_prognostic"])
def test_cli_spp_unit(extra):
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    base = [exe, "1", "300", "64", "--fields", "caller"] + extra
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    spp = subprocess.run(base + ["--spp", "unit"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and spp.returncode == 0, plain.stderr + spp.stderr
    a, b = tsc.oc_table(spp.stdout), tsc.oc_table(plain.stdout)
    assert a == b and len(a) == 1 + (11 if extra else 21) + 1
