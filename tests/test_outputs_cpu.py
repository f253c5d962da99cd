"""The output selection without a GPU: the argument rules of cloudsc_gpu_run_outputs,
cloudsc_cpu_run_outputs and cloudsc_fields_alloc_outputs, and cloudsc_cpu_run_outputs against
cloudsc_cpu_run_precision on the same host state (and the fp64 oracle) -- on raw bits, with the ten
diagnostic flux members NULL, or pointing at sentinel-filled arrays that must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca
from host_harness import ALL21, DIAG, KEPT, KLEV, SENTINEL, bits, check_kept, columns, full_fields, plain_run, run_selected

SHAPES = [(300, 64), (100, 16), (70, 32), (1, 1), (300, 300)]


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


def test_the_selection_names_ten_and_eleven():
    assert len(DIAG) == 10 and len(KEPT) == 11 and len(ALL21) == 21
    assert set(KEPT) | set(DIAG) == set(ALL21) == {k for _, k in ca.VALIDATED}
    assert all(ca.ALL_FIELDS[n] == "2dh" for n in DIAG)
    assert set(KEPT) == {"plude", "tendency_loc_t", "tendency_loc_q", "tendency_loc_a", "tendency_loc_cld", "pcovptot",
                         "prainfrac_toprfz", "pfplsl", "pfplsn", "pfhpsl", "pfhpsn"}
    assert (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC) == (0, 1)
    with pytest.raises(ValueError):
        ca.selected_outputs(2)


# ---------------------------------------------------------------------------
# argument rules
# ---------------------------------------------------------------------------
def test_gpu_run_outputs_prognostic_rules_need_no_gpu(lib):
    f = full_fields()
    ws = C.c_void_p(0x10)

    def run(prec=ca.FP64, variant=ca.VARIANT_KSEG, outputs=ca.OUTPUTS_PROGNOSTIC, ngptot=100, nproma=16, klev=KLEV,
            fields=f, scratch=ws):
        return lib.cloudsc_gpu_run_outputs(0, None, prec, variant, outputs, ngptot, nproma, klev,
                                           C.byref(fields) if fields is not None else None, scratch)
    for outputs in (2, -1, 99):
        assert run(outputs=outputs) == ca.EINVAL
    for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, 77, ca.VARIANT_KSEG | 0x1000,
                    ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM, ca.VARIANT_KCACHE | ca.FP32_EXACT_LIBM):
        assert run(variant=variant) == ca.EINVAL
        assert run(prec=ca.FP32, variant=variant) == ca.EINVAL
    assert run(prec=99) == ca.EINVAL
    assert run(ngptot=0) == ca.EINVAL
    assert run(nproma=0) == ca.EINVAL
    assert run(klev=1) == ca.EINVAL
    assert run(variant=ca.VARIANT_KCACHE, nproma=257) == ca.EINVAL
    assert run(fields=None) == ca.EINVAL
    assert run(scratch=None) == ca.EINVAL               # KSEG needs its workspace
    for missing in KEPT + ("pt", "paph", "ktype"):      # a kept output or an input missing
        assert run(fields=full_fields(without=(missing,))) == ca.EINVAL, missing


def test_gpu_run_outputs_all_keeps_the_rules_of_gpu_run(lib):
    """CLOUDSC_OUTPUTS_ALL is cloudsc_gpu_run: every argument error returns what cloudsc_gpu_run returns for it
    (where there is no device, cloudsc_gpu_run's answer to that).  Only calls that can never launch."""
    ws = C.c_void_p(0x10)
    f = full_fields()
    cases = [dict(prec=99), dict(variant=77), dict(variant=ca.VARIANT_KSEG | 0x1000), dict(ngptot=0), dict(nproma=0),
             dict(klev=1), dict(variant=ca.VARIANT_KCACHE, nproma=257), dict(fields=None),
             dict(fields=full_fields(without=("pfsqlf",))), dict(fields=full_fields(without=("pfplsl",))),
             dict(fields=full_fields(without=DIAG)),     # ALL needs all 21 members
             dict(prec=ca.MIXED, variant=ca.VARIANT_SCC)]
    for kw in cases:
        a = dict(prec=ca.FP64, variant=ca.VARIANT_KSEG, ngptot=100, nproma=16, klev=KLEV, fields=f)
        a.update(kw)
        fp = C.byref(a["fields"]) if a["fields"] is not None else None
        want = lib.cloudsc_gpu_run(0, None, a["prec"], a["variant"], a["ngptot"], a["nproma"], a["klev"], fp, ws)
        got = lib.cloudsc_gpu_run_outputs(0, None, a["prec"], a["variant"], ca.OUTPUTS_ALL, a["ngptot"], a["nproma"],
                                          a["klev"], fp, ws)
        assert got == want and got != 0, kw


def test_cpu_run_outputs_rules(lib, ds):
    f = full_fields()
    p = ca.Params.from_dict(ds.params)

    def run(prec=ca.FP64, outputs=ca.OUTPUTS_PROGNOSTIC, ngptot=100, nproma=16, klev=KLEV, params=p, fields=f):
        return lib.cloudsc_cpu_run_outputs(1, prec, outputs, ngptot, nproma, klev,
                                           C.byref(params) if params is not None else None,
                                           C.byref(fields) if fields is not None else None)
    for outputs in (2, -1, 99):
        assert run(outputs=outputs) == ca.EINVAL
    for outputs in (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC):
        assert run(outputs=outputs, prec=ca.FP32) == ca.EINVAL   # the fp32 arithmetic has no host form
        assert run(outputs=outputs, prec=99) == ca.EINVAL
        assert run(outputs=outputs, ngptot=0) == ca.EINVAL
        assert run(outputs=outputs, nproma=0) == ca.EINVAL
        assert run(outputs=outputs, klev=1) == ca.EINVAL
        assert run(outputs=outputs, params=None) == ca.EINVAL
        assert run(outputs=outputs, fields=None) == ca.EINVAL
        assert run(outputs=outputs, fields=full_fields(without=("tendency_loc_t",))) == ca.EINVAL
        assert run(outputs=outputs, fields=full_fields(without=("pfhpsn",))) == ca.EINVAL
    assert run(outputs=ca.OUTPUTS_ALL, fields=full_fields(without=("pfsqitur",))) == ca.EINVAL   # ALL needs all 21
    bad = ca.Params.from_dict(ds.params)
    bad.ncldtop = 1
    assert run(params=bad) == ca.EINVAL


def test_fields_alloc_outputs_rules_need_no_gpu(lib):
    f, rep = ca.Fields(), ca.Placement()

    def alloc(flags=ca.PLACE_NONE, outputs=ca.OUTPUTS_PROGNOSTIC, fields=f, prec=ca.FP64, ngptot=100, nproma=16):
        return lib.cloudsc_fields_alloc_outputs(0, prec, ngptot, nproma, KLEV, flags, outputs,
                                                C.byref(fields) if fields is not None else None, C.byref(rep))
    for outputs in (2, -1, 99):
        assert alloc(outputs=outputs) == ca.EINVAL
    for outputs in (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC):
        assert alloc(outputs=outputs, flags=4) == ca.EINVAL
        assert alloc(outputs=outputs, fields=None) == ca.EINVAL
    # the other argument errors are cloudsc_fields_alloc's own, with its own code
    for kw in (dict(prec=99), dict(ngptot=0), dict(nproma=0)):
        a = dict(prec=ca.FP64, ngptot=100, nproma=16)
        a.update(kw)
        want = lib.cloudsc_fields_alloc(0, a["prec"], a["ngptot"], a["nproma"], KLEV, ca.PLACE_NONE, C.byref(f),
                                        C.byref(rep))
        assert want != 0
        for outputs in (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC):
            assert alloc(outputs=outputs, **kw) == want, kw


# ---------------------------------------------------------------------------
# cloudsc_cpu_run_outputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("diag", ["null", "sentinel"])
@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED])
@pytest.mark.parametrize("ngptot,nproma", SHAPES)
def test_cpu_run_outputs_prognostic_bitwise(ds, oracle_mod, ngptot, nproma, precision, diag):
    ref = plain_run(ds, "ds", ngptot, nproma, precision)
    got = run_selected(ds, ngptot, nproma, precision, ca.OUTPUTS_PROGNOSTIC, diag)
    check_kept(got, ref, ngptot, nproma)
    for n in DIAG:
        if diag == "sentinel":
            assert (bits(got[n]) == SENTINEL).all(), n       # every byte kept
    if precision == ca.FP64:
        ost, _ = oracle_mod.run_oracle(ds, ngptot, nproma)
        for k in KEPT:
            assert np.array_equal(bits(columns(got[k], ngptot)), bits(columns(ost.arrays[k], ngptot))), k


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED])
def test_cpu_run_outputs_prognostic_with_aerosols(ds, oracle_mod, precision):
    import make_fixtures as mf
    s = mf.with_aerosols(ds)
    ref = plain_run(s, "aerosol", 300, 64, precision)
    got = run_selected(s, 300, 64, precision, ca.OUTPUTS_PROGNOSTIC, "null")
    check_kept(got, ref, 300, 64)
    if precision == ca.FP64:
        ost, _ = oracle_mod.run_oracle(s, 300, 64)
        for k in KEPT:
            assert np.array_equal(bits(columns(got[k], 300)), bits(columns(ost.arrays[k], 300))), k


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED])
def test_cpu_run_outputs_prognostic_shallow_column(ds, precision):
    """KLEV 3 (the bottom three levels as a column of their own), the physics on at every level but the first."""
    import make_fixtures as mf
    s = mf.sliced_levels(ds, ds.klev - 3)
    s.params["ncldtop"] = 2
    assert s.klev == 3
    ref = plain_run(s, "shallow", 100, 16, precision)
    check_kept(run_selected(s, 100, 16, precision, ca.OUTPUTS_PROGNOSTIC, "null"), ref, 100, 16)
    check_kept(run_selected(s, 100, 16, precision, ca.OUTPUTS_PROGNOSTIC, "sentinel"), ref, 100, 16)


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED])
@pytest.mark.parametrize("ngptot,nproma", [(300, 64), (100, 16)])
def test_cpu_run_outputs_all_is_cpu_run_precision(ds, ngptot, nproma, precision):
    ref = plain_run(ds, "ds", ngptot, nproma, precision)
    got = run_selected(ds, ngptot, nproma, precision, ca.OUTPUTS_ALL, "state")
    check_kept(got, ref, ngptot, nproma, names=ALL21)
