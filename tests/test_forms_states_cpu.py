"""The states of tests/form_state_cases.py without a GPU: what the fp64 oracle must show on each of them
(rain, rain freezing, land and sea; the negative controls), and the host twins of two kernel forms --
cloudsc_cpu_run_outputs(PROGNOSTIC) and cloudsc_cpu_run_tendbuf, which compile the phase functions the
device forms compile -- on every state: on raw bits against cloudsc_cpu_run_precision, the fp64 oracle and
the mixed-precision contract, with the NULL and sentinel variants and the padding checks of
tests/test_outputs_cpu.py and tests/test_tendbuf_cpu.py."""
import numpy as np
import pytest

import cloudsc_amd as ca
import form_state_cases as fs
import mixed_expected as mx
import tendbuf_cases as tb
import host_harness as oc

N = fs.NGPTOT
SHAPES = [(N, 64), (N, 16)]
PRECISIONS = {"fp64": ca.FP64, "mixed": ca.MIXED}


# ---------------------------------------------------------------------------
# the states are what they are said to be
# ---------------------------------------------------------------------------
def test_the_table_names_the_states():
    assert len(fs.STATES) == len(set(fs.STATES)) == 23
    assert {fs.base_of(n) for n in fs.STATES} == {"ds", "W", "M"}
    for n in fs.STATES:
        assert ("rain" in fs.ACTIVITY[n]) != ("no_rain" in fs.ACTIVITY[n]), n
        assert "land_sea" in fs.ACTIVITY[n] or fs.base_of(n) == "ds", n       # every W- and M-based state
    assert {n for n in fs.STATES if "toprfz" in fs.ACTIVITY[n]} == {n for n in fs.STATES if fs.base_of(n) == "M"}


def test_goldens_show_what_the_table_expects(scenarios):
    """The committed outputs of the reference kernel on W and M: the figures the activity checks start from."""
    w, m = scenarios["W"].reference, scenarios["M"].reference
    assert np.count_nonzero(w["pfplsl"]) == fs.GOLDEN_W_PFPLSL_NONZERO
    assert np.count_nonzero(w["tendency_loc_cld"][fs.QR]) > 0
    assert np.count_nonzero(m["prainfrac_toprfz"] > 0) == fs.GOLDEN_M_TOPRFZ_COLUMNS == scenarios["M"].klon


@pytest.mark.parametrize("name", fs.STATES)
def test_state_activity(ds, scenarios, oracle_mod, name):
    s = fs.dataset(name, ds, scenarios)
    assert s.klev == fs.KLEV_OF.get(name, 137) and s.klon == N
    assert fs.uses_aerosols(s) == (name == "aerosol_W")
    out = fs.oracle_outputs(oracle_mod, name, s)
    assert fs.activity_failures(name, s, out) == []
    if name in ("W", "M"):                  # the oracle on the committed inputs gives the committed outputs
        gold = scenarios[name].reference
        assert all(np.array_equal(tb.bits(out[k]), tb.bits(gold[k])) for k in fs.NAMES)
    if name == "aerosol_W":                 # the aerosol inputs matter where there is rain and melting
        w = fs.oracle_outputs(oracle_mod, "W", fs.dataset("W", ds, scenarios))
        assert not np.array_equal(out["pfplsn"], w["pfplsn"])
        assert not np.array_equal(out["tendency_loc_cld"][fs.QR], w["tendency_loc_cld"][fs.QR])


# ---------------------------------------------------------------------------
# the host forms on every state
# ---------------------------------------------------------------------------
def expected_bits(oracle_mod, name, s, precision):
    """{field: [..][N]} the form must give: the fp64 oracle's bits, or the mixed-precision contract's."""
    if precision == ca.FP64:
        return fs.oracle_outputs(oracle_mod, name, s)
    return mx.expected(oracle_mod, s, N, fs.ORACLE_NPROMA, key="forms:" + name)


def differing(got, exp, ngptot, names):
    return [k for k in names if not np.array_equal(tb.bits(oc.columns(got[k], ngptot)), tb.bits(exp[k]))]


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("name", fs.STATES)
def test_cpu_prognostic_on_state(ds, scenarios, oracle_mod, name, precision):
    s = fs.dataset(name, ds, scenarios)
    exp = expected_bits(oracle_mod, name, s, PRECISIONS[precision])
    for ngptot, nproma in SHAPES:
        ref = oc.plain_run(s, "forms:" + name, ngptot, nproma, PRECISIONS[precision])
        assert differing(ref, exp, ngptot, oc.ALL21) == [], (nproma, "cloudsc_cpu_run_precision")
        for diag in ("null", "sentinel"):
            got = oc.run_selected(s, ngptot, nproma, PRECISIONS[precision], ca.OUTPUTS_PROGNOSTIC, diag)
            oc.check_kept(got, ref, ngptot, nproma)
            assert differing(got, exp, ngptot, oc.KEPT) == [], (nproma, diag)
            if diag == "sentinel":
                assert all((oc.bits(got[n]) == oc.SENTINEL).all() for n in oc.DIAG), nproma
            if fs.rain_active(name):
                assert np.count_nonzero(oc.columns(got["pfplsl"], ngptot)) > 0


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("name", fs.STATES)
def test_cpu_tendbuf_on_state(ds, scenarios, oracle_mod, name, precision):
    s = fs.dataset(name, ds, scenarios)
    exp = expected_bits(oracle_mod, name, s, PRECISIONS[precision])
    for ngptot, nproma in SHAPES:
        got = oc.run_tendbuf_checked(s, ngptot, nproma, PRECISIONS[precision], 11, "permuted", key="forms:" + name)
        assert differing(got, exp, ngptot, fs.NAMES) == [], nproma
