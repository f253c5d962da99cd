"""The combined kernel form -- the tendency buffers with the prognostic outputs, KForm<..., kFormTb |
kFormProg> -- on states where levels and lanes differ: every state of tests/form_state_cases.py, in fp64,
fp32 and mixed, on KCACHE and KSEG (default schedule, and 3 segments on 3 workgroups), at 100 columns in
blocks of 64 (unpacked) and of 16 (packed, four blocks per wave), compared on raw bits with the plain
unpacked kernel on the same inputs in separate arrays -- on the device, BUFFER_LOC read in place
(cloudsc_fields_compare_tendbuf), and on the host with the sentinel checks; the plain run itself is pinned
to the oracle (fp64) and the mixed-precision contract (mixed).  On the rain-active states the carried rain
flux must reach pfplsl: a form whose carried flux reads as zero passes every dry state."""
import numpy as np
import pytest

import cloudsc_amd as ca
import form_state_cases as fs
import gpu_harness as fg
from gpu_harness import KEPT, ProgPair
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", sorted(fg.PRECISIONS))
@pytest.mark.parametrize("name", fs.STATES)
def test_tendbuf_prognostic_form_on_state(lib, hip, ds, scenarios, oracle_mod, name, precision):
    s, prec = fs.dataset(name, ds, scenarios), fg.PRECISIONS[precision]
    for ngptot, nproma in fs.shapes(name):
        pr = ProgPair(lib, hip, s, ngptot, nproma, prec, fs.TEND_PLANES, fs.ORDER)
        try:
            assert pr.aer == (name == "aerosol_W")
            for variant in fs.VARIANTS:
                pr.fill(("plain",))
                fg.plain_knobs()
                assert fg.pack_of(s, prec, variant, nproma) == 1
                pr.run_both(variant, which=("plain",))
                fg.plain_is_pinned({k: fg.columns(pr.plain.download_raw(k), ngptot) for k in fs.NAMES}, oracle_mod, name, s,
                                   prec)
                for i, sched in enumerate(fs.schedules(name, variant)):
                    pr.fill(("packed",))
                    fg.form_knobs(sched)
                    assert fg.pack_of(s, prec, variant, nproma) == (4 if nproma == 16 else 1)
                    pr.run_form(variant, ca.OUTPUTS_PROGNOSTIC, "kept" if i else "null")
                    assert pr.device_mismatches_inplace(KEPT) == {}, (nproma, variant, sched)
                    assert pr.host_check_form() == [], (nproma, variant, sched)
                    if fs.rain_active(name):          # the carried rain flux reached its output
                        assert np.count_nonzero(fg.columns(pr.packed.download_raw("pfplsl"), ngptot)) > 0, (nproma, variant)
        finally:
            pr.close()
