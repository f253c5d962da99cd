"""The advancing step on the device: cloudsc_gpu_run_advance on KCACHE and KSEG in three precisions, ALL and
SURFACE, against the definition (fp64: the oracle's tendencies and two NumPy lines; mixed: float32 of that on the
widened float inputs; fp32: the device's own ordinary fp32 step and the two lines in float32), its other outputs
against the ordinary step's, against the CPU variant's bits; KSEG with forced hand-offs in place; narrow blocks
packed against unpacked; cloudsc_fields_advance against the CPU pass and step + pass against the fused form; three
in-place steps against the CPU variant; one KSEG workspace for the ordinary and the advancing form; the bytes that
must not change; --advance 1 and --advance 3 through the CLI.  All comparisons are on raw bits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import advance_cases as ac
import cloudsc_amd as ca
from gpu_harness import DIAG, PATTERN, PRECISIONS, VARIANTS, DeviceProblem, columns, host_inputs, raw_bits, validation_table
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

STATE, TMP, LOC = ac.STATE, ac.TMP, ac.LOC
ALL, SURF = ca.OUTPUTS_ALL, ca.OUTPUTS_SURFACE
OTHER = [k for k in ac.NAMES if k not in LOC]


class AdvProblem(DeviceProblem):
    """One set on the device with pattern-filled outputs (a SURFACE set: the ten diagnostic members NULL, the four
    fluxes surface fields) and four pattern-filled arrays for the out-of-place form."""

    def __init__(self, lib, hip, s, ngptot, nproma, precision, outputs=ALL):
        super().__init__(lib, hip, s, ngptot, nproma, precision)
        self.outputs = outputs
        self.host = host_inputs(s, ngptot, nproma, precision, PATTERN, plude_padding=False)
        if outputs == SURF:
            for n in ca.SURFACE_FLUX_FIELDS:
                self.host[n] = np.empty((self.nb, nproma), dtype=self.dt)
                raw_bits(self.host[n])[...] = PATTERN
        self.set = self.device_fields(outputs=outputs)
        self.sel = [k for k in ca.selected_outputs(outputs)]
        self.apart = {x: self.device_array(np.empty_like(self.host[x]), PATTERN) for x in STATE}
        self.fill()

    def fill(self):
        self.set.upload(self.host)
        for x in STATE:
            assert self.hip.hipMemset(self.apart[x], PATTERN, C.c_size_t(self.host[x].nbytes)) == 0

    def fields(self, loc="canary"):
        f = ca.Fields()
        C.memmove(C.byref(f), C.byref(self.set.f), C.sizeof(ca.Fields))
        if loc == "null":
            for n in LOC:
                setattr(f, n, None)
        return f

    def plain(self, variant, stream=None):
        """The ordinary step of the selection on the set: tendency_loc_* and the other outputs."""
        self.checked_step(self.set.f, variant, None if self.outputs == ALL else self.outputs, stream=stream)
        return {k: self.set.download_raw(k) for k in self.sel}

    def advance(self, variant, in_place=True, loc="canary", stream=None):
        f = self.fields(loc)
        adv = ca.Advance.in_place(f) if in_place else ac.adv_struct(self.apart)
        ws = self.scratch(variant)
        ca.gpu_run_advance(f, adv, self.precision, variant, self.outputs, self.ngptot, self.nproma, self.klev,
                           scratch=ws, stream=stream)
        assert self.lib.cloudsc_gpu_check(0, stream, variant & 0xff, ws) == 0
        self.in_place = in_place

    def target(self, x):
        """The array the last advancing step wrote member x to, whole (block layout)."""
        return self.set.download_raw(x) if self.in_place else self.read(self.apart[x], self.host[x])

    def new_state(self):
        return {x: columns(self.target(x), self.ngptot) for x in STATE}

    def kept_wrong(self, loc_written=False):
        """Inputs other than an aliased state member, tendency_loc_*, members outside the selection, the vapour
        plane and padding lanes: the list of what changed."""
        wrong = []
        tail = self.ngptot % self.nproma
        for k, b in self.host.items():
            if getattr(self.set.f, k) is None:
                continue
            out = k in ca.OUTPUT_FIELDS
            aliased = self.in_place and k in STATE
            now = self.set.download_raw(k)
            if (not out and not aliased and k != "plude") or (k in LOC and not loc_written) or (out and k not in self.sel):
                if not np.array_equal(raw_bits(now), raw_bits(b)):
                    wrong.append("%s: changed" % k)
            if tail and (out or aliased) and k != "plude" and not np.array_equal(raw_bits(now[-1][..., tail:]),
                                                                                raw_bits(b[-1][..., tail:])):
                wrong.append("%s: a padding lane was written" % k)
        for x in STATE:
            t = self.target(x)
            if not self.in_place and tail and not (raw_bits(t[-1][..., tail:]) == PATTERN).all():
                wrong.append("adv %s: a padding lane was written" % x)
        vap = self.target("pclv")[:, ac.NSPEC]
        if self.in_place and not np.array_equal(raw_bits(vap), raw_bits(self.host["pclv"][:, ac.NSPEC])):
            wrong.append("the vapour plane was written")
        if not self.in_place and not (raw_bits(vap) == PATTERN).all():
            wrong.append("the vapour plane was written")
        return wrong


def state_differing(got, want, dtype):
    out = []
    for x in STATE:
        sl = slice(0, ac.NSPEC) if x == "pclv" else slice(None)
        if not np.array_equal(raw_bits(got[x][sl]), raw_bits(np.ascontiguousarray(want[x][sl], dtype=dtype))):
            out.append(x)
    return out


def fp32_expectation(p, plain):
    """The two lines in float32 on the problem's float inputs and the ordinary fp32 step's tendency_loc_*."""
    cols = {k: columns(p.host[k], p.ngptot) for k in STATE + TMP}
    loc = {k: columns(plain[k], p.ngptot) for k in LOC}
    return ac.advanced(cols, loc, p.ds.params["ptsphy"], np.float32)


def definition(oracle_mod, name, s, p, plain):
    if p.precision == ca.FP32:
        return fp32_expectation(p, plain)
    new, _ = ac.expected(oracle_mod, name, s, p.precision)
    return {x: ac.wrap(new[x], p.ngptot) for x in STATE}


def others_differing(p, plain):
    return [k for k in OTHER if k in p.sel and not np.array_equal(raw_bits(p.set.download_raw(k)), raw_bits(plain[k]))]


# ---------------------------------------------------------------------------
# the fused form against the definition, the ordinary step's other outputs and the CPU variant
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", list(ac.OUTPUTS))
@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_is_the_definition(lib, hip, ds, scenarios, oracle_mod, variant, precision, outputs):
    s = ac.dataset("W", ds, scenarios)
    p = AdvProblem(lib, hip, s, 100, 64, PRECISIONS[precision], ac.OUTPUTS[outputs])
    try:
        plain = p.plain(VARIANTS[variant])
        p.fill()
        p.advance(VARIANTS[variant], in_place=True, loc="canary")
        got = p.new_state()
        assert state_differing(got, definition(oracle_mod, "W", s, p, plain), p.dt) == []
        assert others_differing(p, plain) == []
        assert p.kept_wrong() == []
        if p.precision != ca.FP32:          # the CPU variant's bits
            st = ca.make_host_state(s, 100, 64, p.precision)
            f = st.fields()
            if p.outputs == SURF:
                for n in DIAG:
                    setattr(f, n, None)
            ca.cpu_run_advance(ca.Params.from_dict(s.params), f, ca.Advance.in_place(f), p.precision, p.outputs, 100,
                               64, s.klev, nthreads=4)
            assert state_differing(got, {x: columns(st.arrays[x], 100) for x in STATE}, p.dt) == []
    finally:
        p.close()


@pytest.mark.parametrize("name,variant,precision", [("M", "kseg", "fp64"), ("aerosol_W", "kcache", "fp64"),
                                                    ("aerosol_W", "kseg", "mixed"), ("ncldtop138", "kseg", "fp64"),
                                                    ("ncldtop40", "kcache", "mixed"), ("klev3", "kseg", "fp64"),
                                                    ("ptsphy_7200", "kseg", "fp32"), ("klev274", "kseg", "fp64")])
def test_fused_on_states_out_of_place(lib, hip, ds, scenarios, oracle_mod, name, variant, precision):
    s = ac.dataset(name, ds, scenarios)
    p = AdvProblem(lib, hip, s, 100, 64, PRECISIONS[precision], SURF)
    try:
        plain = p.plain(VARIANTS[variant])
        p.fill()
        p.advance(VARIANTS[variant], in_place=False, loc="null")
        assert state_differing(p.new_state(), definition(oracle_mod, name, s, p, plain), p.dt) == []
        assert others_differing(p, plain) == []
        assert p.kept_wrong() == []
    finally:
        p.close()


# ---------------------------------------------------------------------------
# KSEG hand-offs in place, sub-blocks, packed narrow blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("shape", [(100, 64), (300, 128), (100, 16)], ids=lambda s: "%dx%d" % s)
def test_kseg_forced_handoffs_in_place(lib, hip, ds, scenarios, oracle_mod, shape, precision):
    """Four segments on three workgroups: every column is handed over three times, and a later segment runs long
    after an earlier one has rewritten its rows of the state.  The bits are the one-shot kernel's out of place."""
    s = ac.dataset("W", ds, scenarios)
    p = AdvProblem(lib, hip, s, *shape, PRECISIONS[precision], SURF)
    try:
        plain = p.plain(ca.VARIANT_KCACHE)
        p.fill()
        p.advance(ca.VARIANT_KCACHE, in_place=False, loc="null")
        ref = p.new_state()
        assert state_differing(ref, definition(oracle_mod, "W", s, p, plain), p.dt) == []
        p.fill()
        ca.kseg_schedule(4, 3)
        p.advance(ca.VARIANT_KSEG, in_place=True, loc="null")
        assert state_differing(p.new_state(), ref, p.dt) == []
        assert others_differing(p, plain) == []
        assert p.kept_wrong() == []
    finally:
        p.close()


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_narrow_blocks_packed_is_unpacked(lib, hip, ds, scenarios, oracle_mod, variant, precision):
    s = ac.dataset("M", ds, scenarios)
    p = AdvProblem(lib, hip, s, 100, 16, PRECISIONS[precision], ALL)
    try:
        assert ca.launch_geometry(p.precision, VARIANTS[variant], 100, 16, s.klev)["pack"] == 4
        ca.narrow_pack(0)
        plain = p.plain(VARIANTS[variant])
        p.fill()
        p.advance(VARIANTS[variant], in_place=True)
        unpacked = p.new_state()
        assert state_differing(unpacked, definition(oracle_mod, "M", s, p, plain), p.dt) == []
        p.fill()
        ca.narrow_pack(1)
        ca.kseg_schedule(3, 2)
        p.advance(VARIANTS[variant], in_place=True)
        assert state_differing(p.new_state(), unpacked, p.dt) == []
        assert others_differing(p, plain) == []
        assert p.kept_wrong() == []
    finally:
        p.close()


# ---------------------------------------------------------------------------
# the separate pass
# ---------------------------------------------------------------------------
def mixed_pass_outside_bound(fused, passed, loc32, ptsphy):
    """Mixed: the fused form adds ptsphy * loc64, the pass ptsphy * float32(loc64), both to the same X0 in double, and
    each narrows its sum once.  |loc64 - loc32| <= 2^-24 |loc64| (2^-150 where loc32 is subnormal), so the two double
    sums are at most ptsphy * |loc32| * 2^-24 (1 + 2^-23) apart plus three double roundings of terms of that size or
    of the sum (2^-52 relative): below ptsphy * (|loc32| * 2^-23 + 2^-149); each narrowing moves its sum by at most
    half a float ulp of the result.  The bound is from the formats alone; the members that break it."""
    bad = []
    for x, l in zip(STATE, LOC):
        sl = slice(0, ac.NSPEC) if x == "pclv" else slice(None)
        a, b = fused[x][sl].astype(np.float64), passed[x][sl].astype(np.float64)
        ulp = np.spacing(np.maximum(np.abs(fused[x][sl]), np.abs(passed[x][sl])).astype(np.float32)).astype(np.float64)
        bound = ptsphy * (np.abs(loc32[l][sl].astype(np.float64)) * 2.0 ** -23 + 2.0 ** -149) + ulp
        if not np.all(np.abs(a - b) <= bound):
            bad.append(x)
    return bad


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("shape", [(100, 64), (300, 128), (1000, 16)], ids=lambda s: "%dx%d" % s)
def test_device_pass_is_the_cpu_pass(lib, hip, ds, shape, precision, in_place):
    """cloudsc_fields_advance after the ordinary step against cloudsc_cpu_fields_advance on the downloaded set,
    whole arrays; in fp64 and fp32 that is the fused form bit for bit."""
    prec = PRECISIONS[precision]
    p = AdvProblem(lib, hip, ds, *shape, prec, ALL)
    try:
        p.plain(ca.VARIANT_KSEG)
        host = {k: p.set.download_raw(k) for k in STATE + TMP + LOC}
        f = p.fields()
        adv = ca.Advance.in_place(f) if in_place else ac.adv_struct(p.apart)
        ca.advance_fields(f, adv, prec, *shape, p.klev)
        p.in_place = in_place
        hf = ca.Fields()
        for k, a in host.items():
            setattr(hf, k, a.ctypes.data)
        target = {x: host[x] for x in STATE}
        if not in_place:
            target = {x: np.empty_like(host[x]) for x in STATE}
            for t in target.values():
                raw_bits(t)[...] = PATTERN
        ca.cpu_advance_fields(ca.Params.from_dict(ds.params), hf, ac.adv_struct(target), prec, *shape, p.klev, nthreads=4)
        for x in STATE:
            assert np.array_equal(raw_bits(p.target(x)), raw_bits(target[x])), x
        assert p.kept_wrong(loc_written=True) == []
        passed = p.new_state()
        p.fill()
        p.advance(ca.VARIANT_KSEG, in_place=in_place, loc="null")
        fused = p.new_state()
        if prec != ca.MIXED:
            assert state_differing(fused, passed, p.dt) == []
        else:
            assert mixed_pass_outside_bound(fused, passed, {k: columns(host[k], p.ngptot) for k in LOC},
                                            ds.params["ptsphy"]) == []
    finally:
        p.close()


# ---------------------------------------------------------------------------
# consecutive steps, one workspace for both forms
# ---------------------------------------------------------------------------
def test_three_steps_in_place_are_the_cpu_variants(lib, hip, ds, scenarios):
    """Three advancing KSEG steps in place on one workspace, an ordinary step of another set between them on the
    same workspace, against three steps of the CPU variant."""
    s = ac.dataset("W", ds, scenarios)
    p = AdvProblem(lib, hip, s, 300, 128, ca.FP64, SURF)
    q = AdvProblem(lib, hip, s, 300, 128, ca.FP64, SURF)
    own = None
    try:
        alone = q.plain(ca.VARIANT_KSEG)
        q.fill()
        own, q.ws = q.ws, p.scratch(ca.VARIANT_KSEG)                 # q launches on p's workspace from here on
        st = ca.make_host_state(s, 300, 128, ca.FP64)
        for n in ca.SURFACE_FLUX_FIELDS:
            st.arrays[n] = np.empty((p.nb, 128), dtype=np.float64)
        f = st.fields()
        for n in DIAG:
            setattr(f, n, None)
        for n in range(3):
            p.advance(ca.VARIANT_KSEG, in_place=True, loc="null")
            shared = q.plain(ca.VARIANT_KSEG)
            assert [k for k in q.sel if not np.array_equal(raw_bits(shared[k]), raw_bits(alone[k]))] == [], n
            q.fill()
            ca.cpu_run_advance(ca.Params.from_dict(s.params), f, ca.Advance.in_place(f), ca.FP64, SURF, 300, 128, s.klev,
                               nthreads=4)
            got = p.new_state()
            assert state_differing(got, {x: columns(st.arrays[x], 300) for x in STATE}, p.dt) == [], n
            assert all(np.all(np.isfinite(a)) for a in got.values()), n
            for k in ("plude", "pcovptot", "prainfrac_toprfz", "pfplsl", "pfplsn"):
                assert np.array_equal(raw_bits(columns(p.set.download_raw(k), 300)), raw_bits(columns(st.arrays[k], 300))), (n, k)
    finally:
        if own is not None:
            q.ws = own
        p.close()
        q.close()


# ---------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------
CLI = os.path.join(os.path.dirname(os.path.abspath(ca.__file__)), "dwarf-cloudsc-amd")
KEPT_ROWS = ["PLUDE", "PCOVPTOT", "PRAINFRAC_TOPRFZ", "PFPLSL", "PFPLSN", "PFHPSL", "PFHPSN"]


def run_cli(*args):
    r = subprocess.run([CLI, "1", "300", "64", "--fields", "caller"] + list(args), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cli_advance_1_validates_what_still_has_a_reference(lib, variant):
    plain = run_cli("--variant", variant)
    out = run_cli("--variant", variant, "--advance", "1")
    rows = [ln.split()[0] for ln in validation_table(out)[1:] if re.search(r"\dD\d", ln)]
    assert rows == [ln.split()[0] for ln in validation_table(plain)[1:] if re.search(r"\dD\d", ln)][:17]
    assert not any(r.lower().startswith("tendency") for r in rows) and len(rows) == 17
    # the rows kept are the ordinary run's rows, character for character
    assert [ln for ln in validation_table(out) if re.search(r"\dD\d", ln)] == \
        [ln for ln in validation_table(plain) if re.search(r"\dD\d", ln)][:17]
    assert "VALIDATION: PASSED" in out
    assert re.search(r"^ ADVANCE: steps=1 ms_per_step=\d+\.\d+ in place", out.splitlines()[-1])
    surf = run_cli("--variant", variant, "--advance", "1", "--outputs", "surface", "--precision", "mixed")
    assert [ln.split()[0] for ln in validation_table(surf)[1:] if re.search(r"\dD\d", ln)] == KEPT_ROWS
    assert surf.splitlines()[-1].startswith(" ADVANCE: steps=1 ")


def test_cli_advance_3_takes_three_steps_and_validates_nothing(lib):
    out = run_cli("--advance", "3", "--outputs", "surface")
    assert [ln for ln in validation_table(out)[1:] if re.search(r"\dD\d", ln)] == []
    assert re.search(r"TIMING: steps=3 ", out)
    assert re.search(r"^ ADVANCE: steps=3 ms_per_step=\d+\.\d+ in place.*nothing validated", out.splitlines()[-1])
    for bad in (["--advance", "0"], ["--advance", "2", "--spp", "unit"], ["--advance", "2", "--outputs", "prognostic"],
                ["--advance", "1", "--fp32-exact-libm", "--precision", "fp32"]):
        r = subprocess.run([CLI, "1", "300", "64", "--fields", "caller"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, bad
