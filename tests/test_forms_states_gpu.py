"""The kernel forms on states where levels and lanes differ.  Each of the tendency buffer form, the
prognostic-outputs form and the packed form is another compiled kernel (KForm<..., FORM>), and the shipped
state -- sub-freezing, sea only, no rain at all -- cannot tell them from the plain kernel on the rain, melting,
freezing and land paths, on the carried rain flux, or at another KLEV.  Here every form runs on every state
of tests/form_state_cases.py, in fp64, fp32 (default exp/pow) and mixed, on KCACHE and KSEG (default
schedule, and 3 segments on 3 workgroups: the carried state crosses the workspace twice), and is compared
on raw bits with the plain unpacked kernel on the same inputs -- on the device (cloudsc_fields_compare) and
again on the host, with the sentinel and padding checks of the harnesses of tests/test_tendbuf_gpu.py,
tests/test_outputs_gpu.py and tests/test_narrow_pack_gpu.py; the plain run itself is pinned to the oracle
(fp64) and to the mixed-precision contract (mixed).

Shapes: 100 columns (each template column once) in blocks of 64 (unpacked, a last block of 36), of 16 (four
blocks per wave, the last group three blocks, the last block four columns) and, for the packed form alone,
of 5 (twelve blocks per wave, 60 lanes)."""
import numpy as np
import pytest

import cloudsc_amd as ca
import form_state_cases as fs
from form_state_cases import ORDER, TEND_PLANES, schedules, shapes
from gpu_harness import PRECISIONS, Pair, Run, Sets, columns, pattern_like, prognostic_parity, widened_bits
from gpu_harness import form_knobs, pack_of, plain_is_pinned, plain_knobs
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

VARIANTS = fs.VARIANTS


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("name", fs.STATES)
def test_tendbuf_form_on_state(lib, hip, ds, scenarios, oracle_mod, name, precision):
    s, prec = fs.dataset(name, ds, scenarios), PRECISIONS[precision]
    for ngptot, nproma in shapes(name):
        pr = Pair(lib, hip, s, ngptot, nproma, prec, TEND_PLANES, ORDER)
        try:
            assert pr.aer == (name == "aerosol_W")
            for variant in VARIANTS:
                pr.fill(("plain",))
                plain_knobs()
                assert pack_of(s, prec, variant, nproma) == 1
                pr.run_both(variant, which=("plain",))
                plain_is_pinned({k: columns(pr.plain.download_raw(k), fs.NGPTOT) for k in fs.NAMES}, oracle_mod, name, s, prec)
                for sched in schedules(name, variant):
                    pr.fill(("packed",))
                    form_knobs(sched)
                    assert pack_of(s, prec, variant, nproma) == (4 if nproma == 16 else 1)
                    pr.run_both(variant, which=("packed",))
                    assert pr.device_mismatches() == {}, (nproma, variant, sched)
                    assert pr.host_check() == [], (nproma, variant, sched)
        finally:
            pr.close()


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("name", fs.STATES)
def test_prognostic_form_on_state(lib, hip, ds, scenarios, oracle_mod, name, precision):
    s, prec = fs.dataset(name, ds, scenarios), PRECISIONS[precision]
    oracle = fs.oracle_outputs(oracle_mod, name, s) if prec == ca.FP64 else None
    for ngptot, nproma in shapes(name):
        st = Sets(lib, hip, s, ngptot, nproma, prec)
        try:
            assert st.aer == (name == "aerosol_W")
            for variant in VARIANTS:
                st.sets["all"].upload(st.host)
                plain_knobs()
                assert pack_of(s, prec, variant, nproma) == 1
                st.run("all", variant, None)
                plain_is_pinned({k: columns(st.sets["all"].download_raw(k), fs.NGPTOT) for k in fs.NAMES}, oracle_mod, name, s,
                                prec)
                for sched in schedules(name, variant):
                    for w in ("null", "kept"):
                        st.sets[w].upload(st.host)
                    form_knobs(sched)
                    assert pack_of(s, prec, variant, nproma) == (4 if nproma == 16 else 1)
                    prognostic_parity(st, variant, oracle, run_all=False)
                    if fs.rain_active(name):          # the carried rain flux reached its output
                        for w in ("null", "kept"):
                            assert np.count_nonzero(columns(st.sets[w].download_raw("pfplsl"), fs.NGPTOT)) > 0, (nproma, w)
        finally:
            st.close()


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("name", fs.STATES)
def test_packed_form_on_state(lib, ds, scenarios, oracle_mod, name, precision):
    """Packed against unpacked on two sets of buffers, each one block longer than the run: the whole buffers
    on the host (the padding lanes and the extra block keep the byte pattern) and cloudsc_fields_compare."""
    s, prec = fs.dataset(name, ds, scenarios), PRECISIONS[precision]
    for ngptot, nproma in shapes(name, packed_form=True):
        off, on = Run(lib, s, ngptot, nproma, prec, extra_blocks=1), Run(lib, s, ngptot, nproma, prec, extra_blocks=1)
        try:
            nb, tail = on.nb, ngptot - (on.nb - 1) * nproma
            for variant in VARIANTS:
                ref = off.launch(variant, 0)
                assert pack_of(s, prec, variant, nproma) == 1
                plain_is_pinned(off.columns(ref), oracle_mod, name, s, prec)
                for sched in schedules(name, variant):
                    out = on.launch(variant, 1, sched)
                    assert pack_of(s, prec, variant, nproma) == 64 // nproma
                    assert on.mismatches(on.df.f, off.df.f, fs.NAMES) == {}, (nproma, variant, sched)
                    for k in fs.NAMES:
                        where = (nproma, variant, sched, k)
                        assert np.array_equal(widened_bits(out[k]), widened_bits(ref[k])), where
                        a, pat = out[k], pattern_like(on.host[k]).astype(np.float64)
                        assert a.shape[0] == nb + 1
                        assert np.array_equal(widened_bits(a[nb:]), widened_bits(pat[nb:])), where + ("past the last block",)
                        assert np.array_equal(widened_bits(a[nb - 1, ..., tail:]), widened_bits(pat[nb - 1, ..., tail:])), \
                            where + ("padding",)
                        assert not np.array_equal(widened_bits(a[:nb - 1]), widened_bits(pat[:nb - 1])), where + ("not written",)
        finally:
            off.close()
            on.close()
