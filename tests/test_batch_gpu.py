"""The batched step on the device: cloudsc_gpu_run_batch over N caller-owned sets against N cloudsc_gpu_run_outputs
(KCACHE) launches on N more sets holding the same inputs, as raw bits of every selected output, whole arrays (so
the padding lanes of a partial last block keep their canary), with the canaries of the members a selection does
not write; per-member parameter sets on shared inputs; nsets == 1; a non-default stream; the CLI's --batch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_cases as bc
import cloudsc_amd as ca
import form_state_cases as fs
from gpu_harness import DIAG, DeviceProblem, raw_bits as bits
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)
from host_harness import validation_table

pytestmark = pytest.mark.gpu

KCACHE = ca.VARIANT_KCACHE


class BatchProblem(DeviceProblem):
    """nsets sets twice on the device -- `single` for the one-shot launches, `batched` for the batch -- set i of
    either holding the state's columns from i * OFFSET on, every output byte the canary.  ALL and PROGNOSTIC sets
    have all 21 members (PROGNOSTIC must leave the ten diagnostic ones alone); SURFACE sets are
    cloudsc_fields_alloc_outputs': the ten NULL, the four surface members small."""

    def __init__(self, lib, hip, ds, nsets, ngptot, nproma, precision, outputs):
        super().__init__(lib, hip, ds, ngptot, nproma, precision)
        self.nsets, self.outputs = nsets, outputs
        self.alloc = ca.OUTPUTS_SURFACE if outputs == ca.OUTPUTS_SURFACE else ca.OUTPUTS_ALL
        self.host = [self.inputs(i * bc.OFFSET) for i in range(nsets)]
        self.single = [self.filled(h) for h in self.host]
        self.batched = [self.filled(h) for h in self.host]

    def inputs(self, col_offset):
        st = ca.make_host_state(self.ds, self.ngptot, self.nproma, self.precision, col_offset)
        out = {}
        for name, a in st.arrays.items():
            a = np.ascontiguousarray(a).copy()
            if name in ca.OUTPUT_FIELDS:
                if self.alloc == ca.OUTPUTS_SURFACE and name in ca.SURFACE_FLUX_FIELDS:
                    a = np.empty((self.nb, self.nproma), dtype=self.dt)
                bits(a)[...] = bc.CANARY
            out[name] = a
        return out

    def filled(self, host):
        d = self.device_fields(outputs=self.alloc)
        d.upload(host)
        return d

    def run_single(self, params=None, stream=None):
        """Set i alone, after cloudsc_gpu_init(params[i]) where given."""
        for i, d in enumerate(self.single):
            if params is not None:
                self.init_params(params[i])
            self.checked_step(d.f, KCACHE, self.outputs, stream=stream)

    def wrong(self):
        """What of the batched sets is not what the single launches left: every member of every set, whole arrays."""
        bad = []
        sel = ca.selected_outputs(self.outputs)
        tail = self.ngptot % self.nproma
        for i, (a, b) in enumerate(zip(self.batched, self.single)):
            for k in ca.selected_outputs(ca.OUTPUTS_ALL):
                if not getattr(a.f, k):
                    assert k in DIAG and k not in sel
                    continue
                got, ref = a.download_raw(k), b.download_raw(k)
                if not np.array_equal(bits(got), bits(ref)):
                    bad.append("set %d %s: differs from the single launch" % (i, k))
                if k not in sel and not (bits(got) == bc.CANARY).all():
                    bad.append("set %d %s: written although not selected" % (i, k))
                if k in sel and k != "plude" and tail and not (bits(got[-1][..., tail:]) == bc.CANARY).all():
                    bad.append("set %d %s: a padding lane was written" % (i, k))
                if k in sel and k != "plude" and (bits(got[0][..., :1]) == bc.CANARY).all():
                    bad.append("set %d %s: not written" % (i, k))
            for k in self.host[i]:                       # the inputs keep every byte
                if k not in ca.OUTPUT_FIELDS and k != "plude" and getattr(a.f, k):
                    if not np.array_equal(bits(a.download_raw(k)), bits(self.host[i][k])):
                        bad.append("set %d %s: an input changed" % (i, k))
        return bad


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_batch_equals_the_single_launches(lib, hip, ds, scenarios, case):
    state, nsets, ngptot, nproma, pack_mode, pack, prec, outs = case
    sd = fs.dataset(state, ds, scenarios)
    precision, outputs = bc.PRECISIONS[prec], bc.OUTPUTS[outs]
    p = BatchProblem(lib, hip, sd, nsets, ngptot, nproma, precision, outputs)
    try:
        ca.narrow_pack(pack_mode)
        geo = ca.launch_geometry(precision, KCACHE, ngptot, nproma, sd.klev, laer=p.aer)
        assert geo["pack"] == pack
        bgeo = ca.batch_launch_geometry(precision, nsets, ngptot, nproma, sd.klev, laer=p.aer)
        assert bgeo["workgroups"] == nsets * geo["workgroups"] and bgeo["wg_threads"] == geo["wg_threads"]
        p.run_single()
        with ca.Batch(p.batched, precision, outputs, ngptot, nproma, sd.klev) as b:   # the device's set
            assert b.nsets == nsets
            b.run()
            assert lib.cloudsc_gpu_check(0, None, KCACHE, None) == 0
            assert p.wrong() == []
        if nsets > 1:    # the sets hold different columns: the members did not all run the same entry
            k = "tendency_loc_t"
            assert not np.array_equal(bits(p.batched[0].download_raw(k)), bits(p.batched[1].download_raw(k)))
    finally:
        p.close()


@pytest.mark.parametrize("prec", sorted(bc.PRECISIONS))
def test_three_parameter_sets_on_one_state(lib, hip, ds, scenarios, prec):
    """Three sets sharing every input (the same pointers; plude and the outputs their own), three parameter sets:
    set i is the single launch after cloudsc_gpu_init(params[i]), and the three differ."""
    sd = fs.dataset("W", ds, scenarios)
    precision, ngptot, nproma = bc.PRECISIONS[prec], 100, 32
    params = bc.perturbed_params(sd.params)
    p = BatchProblem(lib, hip, sd, 3, ngptot, nproma, precision, ca.OUTPUTS_ALL)
    try:
        shared = []
        same = {k: v for k, v in p.host[0].items() if k not in ca.OUTPUT_FIELDS}      # the inputs and plude of set 0
        for i, d in enumerate(p.batched):
            d.upload(same)
            p.single[i].upload(same)
            f = ca.Fields()
            C.memmove(C.byref(f), C.byref(d.f), C.sizeof(ca.Fields))
            for k in p.host[0]:
                if k not in ca.OUTPUT_FIELDS and k != "plude":
                    setattr(f, k, getattr(p.batched[0].f, k))
            shared.append(f)
        p.host = [p.host[0]] * 3
        p.run_single(params)
        p.init_params(params[2])          # whatever the device's set is: a batch with its own sets does not read it
        b = ca.Batch(shared, precision, ca.OUTPUTS_ALL, ngptot, nproma, sd.klev, params=params)
        try:
            b.run()
            assert lib.cloudsc_gpu_check(0, None, KCACHE, None) == 0
        finally:
            b.close()
        assert p.wrong() == []
        out = [{k: d.download_raw(k) for k in ("tendency_loc_t", "tendency_loc_a", "pfplsl")} for d in p.batched]
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert any(not np.array_equal(bits(out[i][k]), bits(out[j][k])) for k in out[i]), (i, j)
    finally:
        p.init_params(ds.params)
        p.close()


@pytest.mark.parametrize("prec", sorted(bc.PRECISIONS))
def test_a_batch_of_one_is_the_single_launch_twice_over(lib, hip, ds, scenarios, prec):
    """nsets == 1 against cloudsc_gpu_run_outputs, and a second run of both: plude is updated in place."""
    sd = fs.dataset("M", ds, scenarios)
    precision = bc.PRECISIONS[prec]
    p = BatchProblem(lib, hip, sd, 1, 100, 32, precision, ca.OUTPUTS_ALL)
    try:
        with ca.Batch(p.batched, precision, ca.OUTPUTS_ALL, 100, 32, sd.klev, params=[sd.params]) as b:
            for _ in range(2):
                p.run_single()
                b.run()
                assert lib.cloudsc_gpu_check(0, None, KCACHE, None) == 0
                assert p.wrong() == []
    finally:
        p.close()


def test_batch_on_a_non_default_stream(lib, hip, ds, scenarios):
    """The launch is asynchronous in its stream; cloudsc_gpu_check on that stream waits for it."""
    sd = fs.dataset("W", ds, scenarios)
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0      # non-blocking: no implicit order with the null stream
    p = BatchProblem(lib, hip, sd, 3, 100, 32, ca.FP64, ca.OUTPUTS_PROGNOSTIC)
    try:
        p.run_single(stream=st)
        hip.hipDeviceSynchronize()                                # the uploads are done before the launch
        with ca.Batch(p.batched, ca.FP64, ca.OUTPUTS_PROGNOSTIC, 100, 32, sd.klev) as b:
            b.run(stream=st)
            assert lib.cloudsc_gpu_check(0, st, KCACHE, None) == 0
            assert p.wrong() == []
    finally:
        hip.hipStreamSynchronize(st)
        p.close()
        hip.hipStreamDestroy(st)


def test_run_batch_refuses_other_variants_on_a_live_batch(lib, hip, ds):
    p = BatchProblem(lib, hip, ds, 2, 64, 64, ca.FP64, ca.OUTPUTS_ALL)
    try:
        with ca.Batch(p.batched, ca.FP64, ca.OUTPUTS_ALL, 64, 64, ds.klev) as b:
            for v in (ca.VARIANT_KSEG, ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, KCACHE | ca.FP32_EXACT_LIBM, 0):
                with pytest.raises(ca.CloudscError) as e:
                    b.run(v)
                assert e.value.code == ca.EINVAL
        assert all((bits(d.download_raw("pcovptot")) == bc.CANARY).all() for d in p.batched)   # nothing ran
    finally:
        p.close()


CLI = os.path.join(os.path.dirname(os.path.abspath(ca.__file__)), "dwarf-cloudsc-amd")


def test_cli_batch_prints_the_table_of_the_columns_together():
    def rows(*args):
        r = subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "VALIDATION: PASSED" in r.stdout
        return [ln for ln in validation_table(r.stdout)[1:] if re.search(r"\dD\d", ln)], r.stdout
    batch, out = rows("1", "300", "32", "--fields", "caller", "--batch", "3", "--variant", "kcache")
    whole, _ = rows("1", "900", "32", "--fields", "caller", "--variant", "kcache")
    assert len(whole) == 21 and batch == whole
    assert re.search(r"^ BATCH: sets=3 columns_per_set=300 ", out, re.M)
    assert "NGPTOT=900," in out
