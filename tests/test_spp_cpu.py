"""Per-column parameter multipliers (SPP) without a GPU: that every slot is live in the oracle on state M;
cloudsc_cpu_run_spp with tuples that vary by column against the columns selected from one fp64 oracle run per
tuple with host-scaled parameters, on raw bits; the all-ones identity; NULL members; PROGNOSTIC; the mixed
identity; the argument rules of both entries; the CLI's --variant cpu --spp unit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import form_state_cases as fs
import spp_cases as sp
import host_harness as oc
from host_harness import full_spp, validation_table as oc_table

NAMES = fs.NAMES
N = fs.NGPTOT
DIAG, KEPT = oc.DIAG, oc.KEPT
CANARY = 0xA7
STATES = ["M", "W", "aerosol_W", "nssopt3"]
BLOCKINGS = [64, 16, 128]           # two blocks with a partial last one | narrow blocks | one block wider than ngptot


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


def columns(blocks, ngptot=N):
    return oc.columns(blocks, ngptot)


def oracle_step(oracle_mod):
    return oc.oracle_step(oracle_mod, N, fs.ORACLE_NPROMA)


_expected = {}


def oracle_expected(oracle_mod, name, s):
    """The fp64 expectation of the mixed-tuple run on a state, from four oracle runs, once, read-only."""
    if name not in _expected:
        e = sp.expected_mixed_tuples(oracle_step(oracle_mod), s, N, ca.FP64, NAMES)
        for a in e.values():
            a.setflags(write=False)
        _expected[name] = e
    return _expected[name]


def run_spp(s, nproma, precision, mult, outputs=ca.OUTPUTS_ALL, diag="state", ngptot=N, host=None, nthreads=3):
    """cloudsc_cpu_run_spp on a fresh host state of s with the multiplier arrays `mult` ({slot: array | None});
    every output lane starts as canary bytes.  Returns the state's arrays (the ten diagnostic members replaced
    by what the call was given)."""
    st = ca.make_host_state(s, ngptot, nproma, precision)
    if host is not None:
        for k, a in host.items():
            st.arrays[k][...] = a
    for n in oc.ALL21:
        if n != "plude":
            sp.bits(st.arrays[n])[...] = CANARY
    f = st.fields()
    given = dict(st.arrays)
    for n in DIAG:
        if diag == "null":
            setattr(f, n, None)
            given[n] = None
        elif diag == "canary":
            a = np.empty_like(st.arrays[n])
            sp.bits(a)[...] = CANARY
            setattr(f, n, a.ctypes.data)
            given[n] = a
    before = {k: a.copy() for k, a in mult.items() if a is not None}
    ca.cpu_run_spp(ca.Params.from_dict(s.params), f, sp.spp_struct(mult), precision, outputs, ngptot, nproma, s.klev,
                   nthreads=nthreads)
    for k, a in before.items():             # the multipliers are only read
        assert np.array_equal(sp.bits(a), sp.bits(mult[k])), k
    return given


def differing(got, want, names=NAMES, ngptot=N):
    return [k for k in names if not np.array_equal(sp.bits(columns(got[k], ngptot)), sp.bits(want[k]))]


def padding_written(got, ngptot, nproma, names=NAMES):
    tail = ngptot % nproma
    return [k for k in names if tail and k != "plude" and not (sp.bits(got[k][-1][..., tail:]) == CANARY).all()]


# ---------------------------------------------------------------------------
# the cases are live: asserted from the oracle alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("slot", sp.SLOTS)
def test_every_slot_is_live_in_the_oracle_on_M(ds, scenarios, oracle_mod, slot):
    """Perturbing one slot alone with its T1 value changes output bits in columns of group 1 -- for rclcrit at
    least one land and one sea column -- so a multiplier that never reaches the physics cannot pass below."""
    m = fs.dataset("M", ds, scenarios)
    step = oracle_step(oracle_mod)
    base = step(m)
    pert = step(sp.scaled_dataset(m, sp.only(slot, 1), ca.FP64))
    changed = set()
    for k in NAMES:
        changed |= set(sp.changed_columns(base[k], pert[k]).tolist())
    assert all(np.all(np.isfinite(a)) for a in pert.values())
    mine = sorted(c for c in changed if sp.group(c) == 1)
    assert mine, slot
    if slot == "rclcrit":
        land = m.inputs["plsm"][..., mine] > 0.5
        assert land.any() and (~land).any(), (mine, land)


def test_W_cannot_stand_in_for_M(ds, scenarios, oracle_mod):
    w = fs.dataset("W", ds, scenarios)
    step = oracle_step(oracle_mod)
    base, pert = step(w), step(sp.scaled_dataset(w, sp.only("ramid", 1), ca.FP64))
    assert all(np.array_equal(sp.bits(base[k]), sp.bits(pert[k])) for k in NAMES)


def test_the_tuple_map_mixes_every_block_of_sixteen():
    g = sp.group(np.arange(256))
    for b in range(16):
        assert set(g[16 * b:16 * b + 16].tolist()) == {0, 1, 2, 3}
    assert [int(np.count_nonzero(sp.group(np.arange(N)) == t)) for t in range(4)] == [25, 25, 25, 25]


# ---------------------------------------------------------------------------
# cloudsc_cpu_run_spp, fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nproma", BLOCKINGS)
@pytest.mark.parametrize("name", STATES)
def test_cpu_spp_fp64_is_the_oracle_under_each_columns_tuple(ds, scenarios, oracle_mod, name, nproma):
    s = fs.dataset(name, ds, scenarios)
    want = oracle_expected(oracle_mod, name, s)
    got = run_spp(s, nproma, ca.FP64, sp.multiplier_fields(N, nproma, ca.FP64))
    assert differing(got, want) == []
    assert padding_written(got, N, nproma) == []
    if name == "M":                          # and the perturbation is visible: not the unperturbed step
        plain = oracle_step(oracle_mod)(s)
        assert differing(got, plain) != []


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED])
@pytest.mark.parametrize("nproma", [64, 16])
def test_cpu_spp_all_ones_is_cpu_run_outputs(ds, scenarios, nproma, precision):
    s = fs.dataset("M", ds, scenarios)
    ref = oc.run_selected(s, N, nproma, precision, ca.OUTPUTS_ALL, "state")
    got = run_spp(s, nproma, precision, sp.uniform_fields(N, nproma, precision, sp.TUPLES[0]))
    assert differing(got, {k: columns(ref[k]) for k in NAMES}) == []


@pytest.mark.parametrize("slot", sp.SLOTS)
def test_cpu_spp_one_member_alone(ds, scenarios, slot):
    """One member non-NULL and the others NULL: the run with ones in their place."""
    s = fs.dataset("M", ds, scenarios)
    full = sp.multiplier_fields(N, 64, ca.FP64, tuples=[sp.only(slot, t) for t in range(4)])
    want = run_spp(s, 64, ca.FP64, full)
    got = run_spp(s, 64, ca.FP64, {k: (a if k == slot else None) for k, a in full.items()})
    assert differing(got, {k: columns(want[k]) for k in NAMES}) == []
    ones = run_spp(s, 64, ca.FP64, sp.uniform_fields(N, 64, ca.FP64, sp.TUPLES[0]))
    assert differing(got, {k: columns(ones[k]) for k in NAMES}) != []


@pytest.mark.parametrize("diag", ["null", "canary"])
def test_cpu_spp_prognostic(ds, scenarios, oracle_mod, diag):
    s = fs.dataset("M", ds, scenarios)
    want = oracle_expected(oracle_mod, "M", s)
    got = run_spp(s, 64, ca.FP64, sp.multiplier_fields(N, 64, ca.FP64), ca.OUTPUTS_PROGNOSTIC, diag)
    assert differing(got, want, names=KEPT) == []
    assert padding_written(got, N, 64, names=KEPT) == []
    if diag == "canary":
        for n in DIAG:
            assert (sp.bits(got[n]) == CANARY).all(), n


@pytest.mark.parametrize("name,nproma", [("M", 64), ("aerosol_W", 16)])
def test_cpu_spp_mixed_identity(ds, scenarios, name, nproma):
    """out = (float) fp64_spp_step((double) in, (double) x)."""
    s = fs.dataset(name, ds, scenarios)
    m32 = sp.multiplier_fields(N, nproma, ca.MIXED)
    got = run_spp(s, nproma, ca.MIXED, m32)
    st32 = ca.make_host_state(s, N, nproma, ca.MIXED)
    wide = {k: a.astype(np.float64) for k, a in st32.arrays.items() if k in s.inputs and a.dtype != np.int32}
    m64 = {k: a.astype(np.float64) for k, a in m32.items()}
    want = run_spp(s, nproma, ca.FP64, m64, host=wide)
    bad = [k for k in NAMES
           if not np.array_equal(sp.bits(columns(got[k])), sp.bits(columns(want[k]).astype(np.float32)))]
    assert bad == []


# ---------------------------------------------------------------------------
# argument rules (no launch, no GPU)
# ---------------------------------------------------------------------------
def test_cpu_run_spp_rules(lib, ds):
    f = oc.full_fields()
    p = ca.Params.from_dict(ds.params)

    def run(prec=ca.FP64, outputs=ca.OUTPUTS_ALL, ngptot=100, nproma=16, klev=oc.KLEV, params=p, fields=f,
            spp=full_spp()):
        return lib.cloudsc_cpu_run_spp(1, prec, outputs, ngptot, nproma, klev,
                                       C.byref(params) if params is not None else None,
                                       C.byref(fields) if fields is not None else None,
                                       C.byref(spp) if spp is not None else None)
    assert run(spp=None) == ca.EINVAL
    assert run(spp=full_spp(**{n: None for n in sp.SLOTS})) == ca.EINVAL
    for n in sp.SLOTS:
        assert run(spp=full_spp(**{n: f.plsm})) == ca.EINVAL, n
        assert run(spp=full_spp(**{n: f.pfhpsn})) == ca.EINVAL, n
    assert run(outputs=ca.OUTPUTS_SURFACE) == ca.EINVAL
    for outputs in (2, -1, 99):
        assert run(outputs=outputs) == ca.EINVAL
    for outputs in (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC):
        assert run(outputs=outputs, prec=ca.FP32) == ca.EINVAL
        assert run(outputs=outputs, ngptot=0) == ca.EINVAL
        assert run(outputs=outputs, klev=1) == ca.EINVAL
        assert run(outputs=outputs, params=None) == ca.EINVAL
        assert run(outputs=outputs, fields=None) == ca.EINVAL
        assert run(outputs=outputs, fields=oc.full_fields(without=("pfhpsn",))) == ca.EINVAL
    assert run(fields=oc.full_fields(without=("pfsqlf",))) == ca.EINVAL      # ALL needs all 21


def test_gpu_run_spp_rules_need_no_gpu(lib):
    oc.gpu_run_spp_rules(lib)


# ---------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_cli_spp_unit_on_the_host(precision):
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    base = [exe, "2", "300", "64", "--variant", "cpu", "--precision", precision]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    spp = subprocess.run(base + ["--spp", "unit"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and spp.returncode == 0, plain.stderr + spp.stderr
    a, b = oc_table(spp.stdout), oc_table(plain.stdout)
    assert a == b and len(a) == 1 + 21 + 1


def test_cli_spp_refuses_what_the_form_does_not_have():
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    for extra in (["--variant", "cpu", "--fields", "caller"], ["--variant", "scc", "--fields", "caller"],
                  ["--fields", "tendbuf"], ["--variant", "cpu", "--outputs", "surface"], ["--transfer"], [],
                  ["--fields", "caller", "--precision", "fp32", "--fp32-exact-libm"]):
        r = subprocess.run([exe, "1", "100", "16", "--spp", "unit"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "VALIDATION" not in r.stdout, extra
    r = subprocess.run([exe, "1", "100", "16", "--spp", "half"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
