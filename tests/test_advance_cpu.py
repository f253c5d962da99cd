"""The advancing step without a GPU: cloudsc_cpu_run_advance against the definition (the fp64 oracle's tendencies,
then two NumPy lines; mixed = float32 of that on float64(float32 inputs)) on raw bits; cloudsc_cpu_fields_advance
after the ordinary step against the fused form; in place against out of place; the bytes that must not change;
three consecutive steps; the argument rules of all four entries; the CLI's --variant cpu --advance N.  The CPU variant computes in double only
(CLOUDSC_FP32 is CLOUDSC_EINVAL in every host run form, cloudsc_cpu_run_precision included), so the fp32 arithmetic
is covered here by the pass alone and by the fused form on the device (tests/test_advance_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import advance_cases as ac
import cloudsc_amd as ca
import form_state_cases as fs
import host_harness as hh
from host_harness import full_fields

PRECISIONS = {"fp64": ca.FP64, "mixed": ca.MIXED}
STATE, TMP, LOC = ac.STATE, ac.TMP, ac.LOC
OTHER = [k for k in ac.NAMES if k not in LOC]          # plude, pcovptot, prainfrac_toprfz and the fourteen fluxes


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


class HostCase:
    """One host set for an advancing run: outputs canary-filled, the selection's members only, tendency_loc_*
    NULL ("null") or canary arrays ("canary") or the state's own ("state"); adv in place or four canary arrays."""

    def __init__(self, s, ngptot, nproma, precision, outputs=ca.OUTPUTS_ALL, in_place=True, loc="canary"):
        self.s, self.ngptot, self.nproma, self.precision, self.outputs = s, ngptot, nproma, precision, outputs
        self.st = ca.make_host_state(s, ngptot, nproma, precision)
        self.nb, self.dt = ca.nblocks_of(ngptot, nproma), ca.storage_dtype(precision)
        a = self.st.arrays
        for n in ca.OUTPUT_FIELDS:
            ac.bits(a[n])[...] = ac.CANARY
        if outputs == ca.OUTPUTS_SURFACE:
            for n in ca.SURFACE_FLUX_FIELDS:
                a[n] = np.empty((self.nb, nproma), dtype=self.dt)
                ac.bits(a[n])[...] = ac.CANARY
        self.f = self.st.fields()
        if outputs == ca.OUTPUTS_SURFACE:
            for n in hh.DIAG:
                setattr(self.f, n, None)
        if loc == "null":
            for n in LOC:
                setattr(self.f, n, None)
        self.in_place = in_place
        self.target = {x: a[x] for x in STATE}
        if not in_place:
            self.target = {x: np.empty_like(a[x]) for x in STATE}
            for t in self.target.values():
                ac.bits(t)[...] = ac.CANARY
        self.adv = ac.adv_struct(self.target)
        self.before = {k: v.copy() for k, v in a.items()}
        self.params = ca.Params.from_dict(s.params)

    def run(self, nthreads=3):
        ca.cpu_run_advance(self.params, self.f, self.adv, self.precision, self.outputs, self.ngptot, self.nproma,
                           self.s.klev, nthreads=nthreads)
        return self

    def new_state(self):
        return {x: hh.columns(self.target[x], self.ngptot) for x in STATE}

    def other(self):
        sel = ca.selected_outputs(self.outputs)
        return {k: hh.columns(self.st.arrays[k], self.ngptot) for k in OTHER if k in sel}

    def kept_wrong(self, loc_written=False):
        """What changed that must not have: inputs other than an aliased state member, tendency_loc_* (unless a
        step was meant to fill them), diagnostic members outside the selection, the vapour plane, padding lanes."""
        a, wrong = self.st.arrays, []
        tail = self.ngptot % self.nproma
        sel = ca.selected_outputs(self.outputs)
        for k, b in self.before.items():
            aliased = self.in_place and k in STATE
            out = k in ca.OUTPUT_FIELDS
            if (not out and not aliased and k != "plude") or (k in LOC and not loc_written) or (out and k not in sel):
                if not np.array_equal(ac.bits(a[k]), ac.bits(b)):
                    wrong.append("%s: changed" % k)
            if tail and (out or aliased) and k != "plude" and not np.array_equal(ac.bits(a[k][-1][..., tail:]),
                                                                                ac.bits(b[-1][..., tail:])):
                wrong.append("%s: a padding lane was written" % k)
        for x in STATE:
            t = self.target[x]
            if not self.in_place and tail and not (ac.bits(t[-1][..., tail:]) == ac.CANARY).all():
                wrong.append("adv %s: a padding lane was written" % x)
        vap = self.target["pclv"][:, ac.NSPEC]
        want = self.before["pclv"][:, ac.NSPEC] if self.in_place else None
        if not (np.array_equal(ac.bits(vap), ac.bits(want)) if self.in_place else (ac.bits(vap) == ac.CANARY).all()):
            wrong.append("the vapour plane was written")
        return wrong


def as_dtype(cols, precision):
    return np.ascontiguousarray(cols, dtype=ca.storage_dtype(precision))


def check_against_definition(case, exp_new, exp_other):
    got, other = case.new_state(), case.other()
    bad = [x for x in STATE
           if not np.array_equal(ac.bits(got[x]), ac.bits(as_dtype(ac.wrap(exp_new[x], case.ngptot), case.precision)))]
    bad += [k for k in other
            if not np.array_equal(ac.bits(other[k]), ac.bits(as_dtype(
                ac.wrap(ac.surface_row(k, exp_other[k]) if case.outputs == ca.OUTPUTS_SURFACE else exp_other[k],
                        case.ngptot), case.precision)))]
    assert bad == []
    assert all(np.all(np.isfinite(a)) for a in got.values())


# ---------------------------------------------------------------------------
# the fused form against the definition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", list(ac.OUTPUTS))
@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("name", ac.STATES)
def test_cpu_run_advance_is_the_definition(ds, scenarios, oracle_mod, name, precision, outputs):
    s = ac.dataset(name, ds, scenarios)
    prec = PRECISIONS[precision]
    new, other = ac.expected(oracle_mod, name, s, prec)
    case = HostCase(s, 100, 64, prec, ac.OUTPUTS[outputs], in_place=True, loc="canary").run()
    check_against_definition(case, new, other)
    assert case.kept_wrong() == []
    # the step did something to the state
    assert not np.array_equal(ac.bits(case.st.arrays["pt"]), ac.bits(case.before["pt"]))


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("shape", ac.SHAPES[1:], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["W", "M"])
def test_cpu_run_advance_other_blockings(ds, scenarios, oracle_mod, name, shape, precision):
    s = ac.dataset(name, ds, scenarios)
    prec = PRECISIONS[precision]
    new, other = ac.expected(oracle_mod, name, s, prec)
    case = HostCase(s, *shape, prec, ca.OUTPUTS_SURFACE, in_place=True, loc="null").run(nthreads=2)
    check_against_definition(case, new, other)
    assert case.kept_wrong() == []


def test_above_ncldtop_the_formula_still_applies(ds, scenarios, oracle_mod):
    """NCLDTOP 138: no physics level at all, yet every level is X + ptsphy * tmp (+ ptsphy * loc), and a -0 state
    with a zero incoming tendency becomes +0."""
    s = ac.dataset("ncldtop138", ds, scenarios).copy()
    s.inputs["pa"][0, :] = -0.0
    s.inputs["tendency_tmp_a"][0, :] = 0.0
    st, _ = oracle_mod.run_oracle(s, fs.NGPTOT, fs.ORACLE_NPROMA)
    out = {k: hh.columns(st.arrays[k], fs.NGPTOT) for k in ac.NAMES}
    assert not np.any(out["tendency_loc_a"])
    new = ac.advanced(s.inputs, out, s.params["ptsphy"], np.float64)
    case = HostCase(s, 100, 64, ca.FP64, in_place=True).run()
    got = case.new_state()
    assert [x for x in STATE if not np.array_equal(ac.bits(got[x]), ac.bits(new[x]))] == []
    assert not np.signbit(got["pa"][0]).any() and not got["pa"][0].any()
    assert np.any(new["pt"] != s.inputs["pt"])           # tendency_tmp_t alone moved the temperature


# ---------------------------------------------------------------------------
# in place, out of place, partial aliasing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: "%dx%d" % s)
def test_in_place_equals_out_of_place(ds, scenarios, shape, precision):
    s = ac.dataset("W", ds, scenarios)
    prec = PRECISIONS[precision]
    a = HostCase(s, *shape, prec, ca.OUTPUTS_ALL, in_place=True, loc="null").run()
    b = HostCase(s, *shape, prec, ca.OUTPUTS_ALL, in_place=False, loc="canary").run()
    ga, gb = a.new_state(), b.new_state()
    ga["pclv"], gb["pclv"] = ga["pclv"][:ac.NSPEC], gb["pclv"][:ac.NSPEC]     # (the vapour plane: kept_wrong)
    assert [x for x in STATE if not np.array_equal(ac.bits(ga[x]), ac.bits(gb[x]))] == []
    oa, ob = a.other(), b.other()
    assert [k for k in oa if not np.array_equal(ac.bits(oa[k]), ac.bits(ob[k]))] == []
    assert a.kept_wrong() == [] and b.kept_wrong() == []
    for x in STATE:                                       # out of place: the state itself keeps every byte
        assert np.array_equal(ac.bits(b.st.arrays[x]), ac.bits(b.before[x])), x


def test_partial_aliasing(ds, scenarios):
    """t and clv in place, q and a elsewhere: each of the four is independent."""
    s = ac.dataset("M", ds, scenarios)
    ref = HostCase(s, 100, 64, ca.FP64, in_place=True).run().new_state()
    case = HostCase(s, 100, 64, ca.FP64, in_place=False)
    case.target["pt"], case.target["pclv"] = case.st.arrays["pt"], case.st.arrays["pclv"]
    case.adv = ac.adv_struct(case.target)
    got = case.run().new_state()
    assert [x for x in STATE if not np.array_equal(ac.bits(got[x]), ac.bits(ref[x]))] == []
    for x in ("pq", "pa"):
        assert np.array_equal(ac.bits(case.st.arrays[x]), ac.bits(case.before[x])), x


# ---------------------------------------------------------------------------
# the separate pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["W", "aerosol_W"])
def test_pass_after_step_is_the_fused_form_fp64(ds, scenarios, name, shape, in_place):
    s = ac.dataset(name, ds, scenarios)
    fused = HostCase(s, *shape, ca.FP64, in_place=in_place).run()
    step = HostCase(s, *shape, ca.FP64, in_place=in_place, loc="state")
    ca.cpu_run_outputs(step.params, step.f, ca.FP64, ca.OUTPUTS_ALL, *shape, s.klev, nthreads=2)
    ca.cpu_advance_fields(step.params, step.f, step.adv, ca.FP64, *shape, s.klev, nthreads=2)
    for x in STATE:                                       # whole arrays: padding lanes and the vapour plane included
        assert np.array_equal(ac.bits(step.target[x]), ac.bits(fused.target[x])), x
    assert step.kept_wrong(loc_written=True) == []


def pass_inputs(ngptot, nproma, klev, precision, seed=5):
    """A set for the pass alone: the twelve members, values of both signs and magnitudes, -0 among them."""
    rng = np.random.default_rng(seed)
    nb, dt = ca.nblocks_of(ngptot, nproma), ca.storage_dtype(precision)
    arrays = {}
    for x, t, l in zip(STATE, TMP, LOC):
        shp = (nb, 5, klev, nproma) if x == "pclv" else (nb, klev, nproma)
        arrays[x] = (rng.standard_normal(shp) * 10.0 ** rng.integers(-12, 3, shp)).astype(dt)
        arrays[t] = (rng.standard_normal(shp) * 1e-5).astype(dt)
        arrays[l] = (rng.standard_normal(shp) * 10.0 ** rng.integers(-15, -3, shp)).astype(dt)
        arrays[x][0, ..., 0, :4] = -0.0
        arrays[t][0, ..., 0, :4] = 0.0
        arrays[l][0, ..., 0, :4] = 0.0
    return arrays


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED, ca.FP32], ids=["fp64", "mixed", "fp32"])
def test_pass_against_numpy(ds, precision, in_place):
    """cloudsc_cpu_fields_advance against the two lines: float64 for fp64 and mixed (narrowed once), float32 for
    fp32; a -0 state with zero tendencies becomes +0; vapour plane and padding lanes keep their bytes."""
    ngptot, nproma, klev = 100, 64, 5
    a = pass_inputs(ngptot, nproma, klev, precision)
    before = {k: v.copy() for k, v in a.items()}
    f = ca.Fields()
    for k, v in a.items():
        setattr(f, k, v.ctypes.data)
    target = {x: a[x] for x in STATE}
    if not in_place:
        target = {x: np.empty_like(a[x]) for x in STATE}
        for t in target.values():
            ac.bits(t)[...] = ac.CANARY
    params = ca.Params.from_dict(ds.params)
    ca.cpu_advance_fields(params, f, ac.adv_struct(target), precision, ngptot, nproma, klev, nthreads=2)
    work = np.float32 if precision == ca.FP32 else np.float64
    cols = {k: hh.columns(v, ngptot) for k, v in before.items()}
    with np.errstate(over="ignore", under="ignore"):
        want = {x: ac.two_lines(cols[x], cols[t], cols[l], ds.params["ptsphy"], work).astype(a[x].dtype)
                for x, t, l in zip(STATE, TMP, LOC)}
    tail = ngptot % nproma
    for x in STATE:
        got = hh.columns(target[x], ngptot)
        sl = slice(0, ac.NSPEC) if x == "pclv" else slice(None)
        assert np.array_equal(ac.bits(got[sl]), ac.bits(want[x][sl])), x
        keep = before[x] if in_place else None
        pad = target[x][-1][..., tail:]
        assert np.array_equal(ac.bits(pad), ac.bits(keep[-1][..., tail:])) if in_place else (ac.bits(pad) == ac.CANARY).all()
    vap = target["pclv"][:, ac.NSPEC]
    assert np.array_equal(ac.bits(vap), ac.bits(before["pclv"][:, ac.NSPEC])) if in_place else (ac.bits(vap) == ac.CANARY).all()
    got_t = hh.columns(target["pt"], ngptot)
    assert not np.signbit(got_t[0, :4]).any() and not got_t[0, :4].any()
    for k in TMP + LOC:
        assert np.array_equal(ac.bits(a[k]), ac.bits(before[k])), k


def test_mixed_pass_differs_from_the_fused_form_only_by_the_rounding_of_loc(ds, scenarios):
    """Documented, not hidden behind a tolerance: the fused mixed form takes the double tendency, the pass the
    stored float.  The pass is exactly the two lines on the stored floats; the fused form is the definition."""
    s = ac.dataset("W", ds, scenarios)
    step = HostCase(s, 100, 64, ca.MIXED, in_place=False, loc="state")
    ca.cpu_run_outputs(step.params, step.f, ca.MIXED, ca.OUTPUTS_ALL, 100, 64, s.klev, nthreads=2)
    ca.cpu_advance_fields(step.params, step.f, step.adv, ca.MIXED, 100, 64, s.klev, nthreads=2)
    cols = {k: hh.columns(step.st.arrays[k], 100) for k in STATE + TMP + LOC}
    for x, t, l in zip(STATE, TMP, LOC):
        sl = slice(0, ac.NSPEC) if x == "pclv" else slice(None)
        want = ac.two_lines(cols[x][sl], cols[t][sl], cols[l][sl], s.params["ptsphy"], np.float64).astype(np.float32)
        assert np.array_equal(ac.bits(hh.columns(step.target[x], 100)[sl]), ac.bits(want)), x


# ---------------------------------------------------------------------------
# consecutive steps
# ---------------------------------------------------------------------------
def test_three_steps_in_place_are_three_rounds_of_step_and_pass(ds, scenarios):
    s = ac.dataset("W", ds, scenarios)
    fused = HostCase(s, 100, 64, ca.FP64, ca.OUTPUTS_SURFACE, in_place=True, loc="null")
    step = HostCase(s, 100, 64, ca.FP64, ca.OUTPUTS_ALL, in_place=True, loc="state")
    for n in range(3):
        fused.run()
        ca.cpu_run_outputs(step.params, step.f, ca.FP64, ca.OUTPUTS_ALL, 100, 64, s.klev, nthreads=2)
        ca.cpu_advance_fields(step.params, step.f, step.adv, ca.FP64, 100, 64, s.klev, nthreads=2)
        for x in STATE:
            assert np.array_equal(ac.bits(fused.target[x]), ac.bits(step.target[x])), (n, x)
            assert np.all(np.isfinite(hh.columns(fused.target[x], 100))), (n, x)
        for k in ("plude", "pcovptot", "prainfrac_toprfz"):
            assert np.array_equal(ac.bits(fused.st.arrays[k]), ac.bits(step.st.arrays[k])), (n, k)
    assert not np.array_equal(ac.bits(fused.st.arrays["pq"]), ac.bits(fused.before["pq"]))


# ---------------------------------------------------------------------------
# the argument rules (no launch: with and without a GPU)
# ---------------------------------------------------------------------------
def full_adv(f, **kw):
    adv = ca.Advance(f.pt, f.pq, f.pa, f.pclv)
    for k, v in kw.items():
        setattr(adv, k, v)
    return adv


def ref_of(x):
    return C.byref(x) if x is not None else None


def test_run_advance_rules(lib, ds):
    f = full_fields()
    p = ca.Params.from_dict(ds.params)
    ws = C.c_void_p(0x10)

    def cpu(prec=ca.FP64, outputs=ca.OUTPUTS_SURFACE, ngptot=100, nproma=16, klev=137, fields=f, adv="own"):
        adv = full_adv(fields or f) if adv == "own" else adv
        return lib.cloudsc_cpu_run_advance(1, prec, outputs, ngptot, nproma, klev, C.byref(p), ref_of(fields),
                                           ref_of(adv))

    def gpu(prec=ca.FP64, variant=ca.VARIANT_KSEG, outputs=ca.OUTPUTS_SURFACE, ngptot=100, nproma=16, klev=137,
            fields=f, adv="own", scratch=ws):
        adv = full_adv(fields or f) if adv == "own" else adv
        return lib.cloudsc_gpu_run_advance(0, None, prec, variant, outputs, ngptot, nproma, klev, ref_of(fields),
                                           ref_of(adv), scratch)
    before = lib.cloudsc_last_hip_error()
    for run in (cpu, gpu):
        for outputs in (ca.OUTPUTS_ALL, ca.OUTPUTS_SURFACE):
            assert run(outputs=outputs, adv=None) == ca.EINVAL
            for m in ac.ADV:                                                   # a NULL member
                assert run(outputs=outputs, adv=full_adv(f, **{m: None})) == ca.EINVAL
            assert run(outputs=outputs, adv=full_adv(f, t=f.pq)) == ca.EINVAL            # another state member
            assert run(outputs=outputs, adv=full_adv(f, q=f.pap)) == ca.EINVAL           # a non-state member
            # adv with the tendency planes: the entries take no tend_planes, cml or spp (the form bits refuse kFormAdv
            # beside kFormTb, kFormCml, kFormSpp), and a tendency member is no place for the new state
            assert run(outputs=outputs, adv=full_adv(f, a=f.tendency_tmp_a)) == ca.EINVAL
            assert run(outputs=outputs, adv=full_adv(f, clv=f.tendency_loc_cld)) == ca.EINVAL
            assert run(outputs=outputs, adv=full_adv(f, t=0x7000, q=0x7000)) == ca.EINVAL   # two adv members equal
            assert run(outputs=outputs, fields=None) == ca.EINVAL
            assert run(outputs=outputs, fields=full_fields(without=("pt",))) == ca.EINVAL
            assert run(outputs=outputs, ngptot=0) == ca.EINVAL
            assert run(outputs=outputs, nproma=0) == ca.EINVAL
            assert run(outputs=outputs, klev=1) == ca.EINVAL
            assert run(outputs=outputs, prec=99) == ca.EINVAL
        assert run(outputs=ca.OUTPUTS_PROGNOSTIC) == ca.EINVAL                # PROGNOSTIC alone
        for outputs in (2, 4, -1, 99):
            assert run(outputs=outputs) == ca.EINVAL
        assert run(outputs=ca.OUTPUTS_ALL, fields=full_fields(without=("pfsqlf",))) == ca.EINVAL
    assert cpu(prec=ca.FP32) == ca.EINVAL                                      # the fp32 arithmetic has no host form
    for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, 77, ca.VARIANT_KSEG | 0x1000,
                    ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM, ca.VARIANT_KCACHE | ca.FP32_EXACT_LIBM):
        for prec in (ca.FP64, ca.FP32, ca.MIXED):
            assert gpu(prec=prec, variant=variant) == ca.EINVAL
    assert gpu(scratch=None) == ca.EINVAL
    assert gpu(variant=ca.VARIANT_KCACHE, nproma=257) == ca.EINVAL
    assert lib.cloudsc_last_hip_error() == before
    # tendency_loc_* may be NULL: such a set passes every rule (the run itself: the tests above)
    st = HostCase(ds, 20, 16, ca.FP64, ca.OUTPUTS_SURFACE, loc="null")
    assert all(getattr(st.f, n) is None for n in LOC)
    st.run(nthreads=1)


def test_fields_advance_rules(lib, ds):
    f = full_fields()
    p = ca.Params.from_dict(ds.params)

    def cpu(prec=ca.FP64, ngptot=100, nproma=16, klev=137, fields=f, adv="own", params=p):
        adv = full_adv(fields or f) if adv == "own" else adv
        return lib.cloudsc_cpu_fields_advance(1, prec, ngptot, nproma, klev, ref_of(params), ref_of(fields), ref_of(adv))

    def gpu(prec=ca.FP64, ngptot=100, nproma=16, klev=137, fields=f, adv="own"):
        adv = full_adv(fields or f) if adv == "own" else adv
        return lib.cloudsc_fields_advance(0, None, prec, ngptot, nproma, klev, ref_of(fields), ref_of(adv))
    before = lib.cloudsc_last_hip_error()
    for run in (cpu, gpu):
        assert run(adv=None) == ca.EINVAL
        assert run(fields=None) == ca.EINVAL
        for m in ac.ADV:
            assert run(adv=full_adv(f, **{m: None})) == ca.EINVAL
        for n in STATE + TMP + LOC:
            assert run(fields=full_fields(without=(n,))) == ca.EINVAL
        assert run(adv=full_adv(f, t=f.pq)) == ca.EINVAL
        assert run(adv=full_adv(f, clv=f.tendency_loc_cld)) == ca.EINVAL
        assert run(adv=full_adv(f, a=0x7000, q=0x7000)) == ca.EINVAL
        assert run(prec=99) == ca.EINVAL
        assert run(ngptot=0) == ca.EINVAL
        assert run(nproma=0) == ca.EINVAL
        assert run(nproma=(1 << 24) + 1) == ca.EINVAL
        assert run(klev=0) == ca.EINVAL
    assert cpu(params=None) == ca.EINVAL
    assert lib.cloudsc_last_hip_error() == before


# ---------------------------------------------------------------------------
# the CLI on the host variant
# ---------------------------------------------------------------------------
CLI = os.path.join(os.path.dirname(os.path.abspath(ca.__file__)), "dwarf-cloudsc-amd")


def run_cli(*args, ok=True):
    r = subprocess.run([CLI, "2", "100", "16", "--variant", "cpu"] + list(args), capture_output=True, text=True,
                       timeout=120)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout


def data_rows(out):
    return [ln for ln in hh.validation_table(out)[1:] if re.search(r"\dD\d", ln)]


def test_cli_cpu_advance():
    plain, one = run_cli(), run_cli("--advance", "1")
    assert data_rows(one) == data_rows(plain)[:17] and len(data_rows(plain)) == 21     # the tendencies have no row
    assert "VALIDATION: PASSED" in one
    assert re.search(r"^ ADVANCE: steps=1 ms_per_step=\d+\.\d+ in place", one.splitlines()[-1])
    assert "ADVANCE" not in plain
    three = run_cli("--advance", "3", "--outputs", "surface", "--precision", "mixed")
    assert data_rows(three) == [] and re.search(r"TIMING: steps=3 ", three)
    assert re.search(r"^ ADVANCE: steps=3 .*nothing validated", three.splitlines()[-1])
    for bad in (["--advance", "0"], ["--advance", "x"], ["--advance", "2", "--spp", "unit"],
                ["--advance", "1", "--fields", "caller"], ["--advance", "1", "--fields", "tendbuf"]):
        run_cli(*bad, ok=False)
