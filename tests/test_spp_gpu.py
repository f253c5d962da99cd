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
import host_harness as hh
import spp_cases as sp
from gpu_harness import DIAG, DeviceProblem, KEPT, PATTERN, PRECISIONS, VARIANTS, columns, differing, host_inputs
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ALL, PROG = ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC
NAMES = fs.NAMES


class Dev(DeviceProblem):
    """One problem on the device: a field set with all 21 outputs allocated and pattern-filled, the five
    multiplier fields, the KSEG workspace; the device's default parameter set is the state's."""

    def __init__(self, lib, hip, s, ngptot, nproma, precision, mult):
        super().__init__(lib, hip, s, ngptot, nproma, precision)
        self.s = s
        self.host = host_inputs(s, ngptot, nproma, precision, PATTERN)
        self.df = self.device_fields()
        self.mult = mult
        self.dmult = {k: self.device_array(a) for k, a in mult.items()}
        self.spp = ca.Spp(*[self.dmult.get(k) for k in sp.SLOTS])

    def step(self, variant, outputs, spp):
        """One step on freshly uploaded inputs and pattern-filled outputs; {name: block-layout array}."""
        self.df.upload(self.host)
        self.checked_step(self.df.f, variant, outputs, spp=self.spp if spp else None)
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
            if not np.array_equal(sp.bits(self.read(self.dmult[k], a)), sp.bits(a)):
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


def same(a, b, names, ngptot):
    return differing({n: columns(a[n], ngptot) for n in names}, {n: columns(b[n], ngptot) for n in names}, names)


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
        e = sp.expected_mixed_tuples(hh.oracle_step(oracle_mod, ngptot, fs.ORACLE_NPROMA), s, ngptot, ca.FP64, NAMES)
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
        plain = hh.oracle_step(oracle_mod, 100, fs.ORACLE_NPROMA)(s)
        assert [k for k in NAMES if not np.array_equal(sp.bits(columns(first[k], 100)), sp.bits(plain[k]))] == []
    finally:
        d.close()


# ---------------------------------------------------------------------------
# argument rules, the CLI
# ---------------------------------------------------------------------------
def test_argument_rules_on_the_device(lib, hip, ds):
    hh.gpu_run_spp_rules(lib)
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
    a, b = hh.validation_table(spp.stdout), hh.validation_table(plain.stdout)
    assert a == b and len(a) == 1 + (11 if extra else 21) + 1
