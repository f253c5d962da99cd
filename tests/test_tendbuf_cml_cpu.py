"""The cumulative tendency buffer without a GPU: every argument rule of cloudsc_tendbuf_bind_cml,
cloudsc_gpu_run_tendbuf_cml, cloudsc_cpu_run_tendbuf_cml and the two accumulate passes; the host fused form
against NumPy's `cml_old + loc` with loc from cloudsc_cpu_run_tendbuf (fp64, raw bits), the mixed identity
against the fp64 form on widened inputs, the separate pass against NumPy and against the fused form, and the
bytes that must not change: the vapour plane, unbound planes, padding lanes and a canary-filled BUFFER_LOC."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import form_state_cases as fs
import tendbuf_cases as tb
import tendbuf_cml_cases as cm
import host_harness as oc
from host_harness import CANARY, KEPT_OTHER, KLEV, host_set

PROG, SURF, ALL = ca.OUTPUTS_PROGNOSTIC, ca.OUTPUTS_SURFACE, ca.OUTPUTS_ALL


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


def ref_of(p):
    return C.byref(p) if p is not None else None


def no_device():
    try:
        return ca.device_count() == 0
    except ca.CloudscError:
        return True


def full_cml(**kw):
    c = ca.TendCml()
    c.t, c.q, c.a, c.cld = 0x900000, 0x910000, 0x920000, 0x930000
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ---------------------------------------------------------------------------
# argument rules: each returns its code on a machine without a GPU
# ---------------------------------------------------------------------------
def test_bind_cml_rules_and_planes(lib):
    c = ca.TendCml()
    for cml, prec, nproma, klev, buf in ((None, ca.FP64, 16, 5, 64), (c, 99, 16, 5, 64), (c, ca.FP64, 0, 5, 64),
                                         (c, ca.FP64, 16, 0, 64), (c, ca.FP64, 16, 5, None)):
        assert lib.cloudsc_tendbuf_bind_cml(ref_of(cml), prec, nproma, klev, buf) == ca.EINVAL
    for prec, es in ((ca.FP64, 8), (ca.MIXED, 4), (ca.FP32, 4)):
        c = ca.bind_tendbuf_cml(prec, 16, 5, 1 << 20)
        plane = 16 * 5 * es
        assert (c.t, c.a, c.q, c.cld) == tuple((1 << 20) + p * plane for p in
                                               (ca.TENDBUF_T, ca.TENDBUF_A, ca.TENDBUF_Q, ca.TENDBUF_CLD))
    f, c = ca.bind_tendbuf_three(ca.Fields(), ca.FP64, 16, 5, 1 << 20, 1 << 22)
    assert f.tendency_tmp_q == (1 << 20) + ca.TENDBUF_Q * 16 * 5 * 8 and f.tendency_loc_q is None
    assert c.q == (1 << 22) + ca.TENDBUF_Q * 16 * 5 * 8
    f, c = ca.bind_tendbuf_three(ca.Fields(), ca.FP64, 16, 5, 1 << 20, 1 << 22, 1 << 24)
    assert f.tendency_loc_cld == (1 << 24) + ca.TENDBUF_CLD * 16 * 5 * 8


def cml_rule_cases(run, gpu):
    """The contract's errors through one entry point; run(**kw) returns the code."""
    f = oc.full_fields()
    assert run(outputs=ALL) == ca.EINVAL                      # the flux diagnostics go with the separate pass
    for outputs in (2, 4, -1, 99):
        assert run(outputs=outputs) == ca.EINVAL
    for outputs in (PROG, SURF):
        for planes in (7, 65, 0, -1):
            assert run(outputs=outputs, planes=planes) == ca.EINVAL
        assert run(outputs=outputs, cml=None) == ca.EINVAL
        for k in cm.CML:
            assert run(outputs=outputs, cml=full_cml(**{k: None})) == ca.EINVAL, k
            for n in tb.TMP + tb.LOC:                         # a cumulative plane that is a tendency member
                assert run(outputs=outputs, cml=full_cml(**{k: getattr(f, n)})) == ca.EINVAL, (k, n)
        assert run(outputs=outputs, prec=99) == ca.EINVAL
        assert run(outputs=outputs, ngptot=0) == ca.EINVAL
        assert run(outputs=outputs, nproma=0) == ca.EINVAL
        assert run(outputs=outputs, klev=1) == ca.EINVAL
        assert run(outputs=outputs, fields=None) == ca.EINVAL
        for missing in KEPT_OTHER + ("pt", "tendency_tmp_cld", "ktype"):
            assert run(outputs=outputs, fields=oc.full_fields(without=(missing,))) == ca.EINVAL, missing
        if gpu:
            for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, 77, ca.VARIANT_KSEG | 0x1000,
                            ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM, ca.VARIANT_KCACHE | ca.FP32_EXACT_LIBM):
                assert run(outputs=outputs, variant=variant) == ca.EINVAL
                assert run(outputs=outputs, prec=ca.FP32, variant=variant) == ca.EINVAL
            assert run(outputs=outputs, variant=ca.VARIANT_KCACHE, nproma=257) == ca.EINVAL
            assert run(outputs=outputs, scratch=None) == ca.EINVAL           # KSEG needs its workspace
        else:
            assert run(outputs=outputs, prec=ca.FP32) == ca.EINVAL           # the fp32 arithmetic has no host form
            assert run(outputs=outputs, params=None) == ca.EINVAL


def test_gpu_run_tendbuf_cml_rules_need_no_gpu(lib):
    f, c, ws = oc.full_fields(), full_cml(), C.c_void_p(0x10)

    def run(prec=ca.FP64, variant=ca.VARIANT_KSEG, outputs=PROG, ngptot=100, nproma=16, klev=KLEV, planes=8, fields=f,
            cml=c, scratch=ws):
        return lib.cloudsc_gpu_run_tendbuf_cml(0, None, prec, variant, outputs, ngptot, nproma, klev, planes,
                                               ref_of(fields), ref_of(cml), scratch)
    cml_rule_cases(run, gpu=True)
    # what is left is a well-formed call, tendency_loc_* NULL included: without a device it gets as far as asking for one
    if no_device():
        rc = run(fields=oc.full_fields(without=tb.LOC + tuple(oc.DIAG)))
        assert rc != ca.EINVAL and rc != 0


def test_cpu_run_tendbuf_cml_rules(lib, ds):
    f, c, p = oc.full_fields(), full_cml(), ca.Params.from_dict(ds.params)

    def run(prec=ca.FP64, outputs=PROG, ngptot=100, nproma=16, klev=KLEV, planes=8, params=p, fields=f, cml=c):
        return lib.cloudsc_cpu_run_tendbuf_cml(1, prec, outputs, ngptot, nproma, klev, planes, ref_of(params),
                                               ref_of(fields), ref_of(cml))
    cml_rule_cases(run, gpu=False)


@pytest.mark.parametrize("device_form", [False, True])
def test_accumulate_rules_need_no_gpu(lib, device_form):
    f, c = ca.Fields(), full_cml()
    for i, n in enumerate(tb.LOC):
        setattr(f, n, 0x3000 + 0x100 * i)

    def acc(prec=ca.FP64, ngptot=100, nproma=16, klev=3, lpl=8, loc=f, cpl=0, cml=c):
        if device_form:
            return lib.cloudsc_fields_accumulate_tendbuf(0, None, prec, ngptot, nproma, klev, lpl, ref_of(loc), cpl,
                                                         ref_of(cml))
        return lib.cloudsc_cpu_fields_accumulate_tendbuf(1, prec, ngptot, nproma, klev, lpl, ref_of(loc), cpl,
                                                         ref_of(cml))
    for planes in (7, 65, -1, 1):
        assert acc(lpl=planes) == ca.EINVAL
        assert acc(cpl=planes) == ca.EINVAL
    for lpl, cpl in ((8, 0), (0, 11), (11, 8), (0, 0)):
        kw = dict(lpl=lpl, cpl=cpl)
        assert acc(prec=99, **kw) == ca.EINVAL
        assert acc(ngptot=0, **kw) == ca.EINVAL
        assert acc(nproma=0, **kw) == ca.EINVAL
        assert acc(nproma=(1 << 24) + 1, **kw) == ca.EINVAL
        assert acc(klev=0, **kw) == ca.EINVAL
        assert acc(loc=None, **kw) == ca.EINVAL
        assert acc(cml=None, **kw) == ca.EINVAL
        for n in tb.LOC:
            g = ca.Fields()
            C.memmove(C.byref(g), C.byref(f), C.sizeof(ca.Fields))
            setattr(g, n, None)
            assert acc(loc=g, **kw) == ca.EINVAL, n
            for k in cm.CML:
                assert acc(cml=full_cml(**{k: getattr(f, n)}), **kw) == ca.EINVAL, (k, n)
        for k in cm.CML:
            assert acc(cml=full_cml(**{k: None}), **kw) == ca.EINVAL, k


# ---------------------------------------------------------------------------
# the host fused form
# ---------------------------------------------------------------------------
def fused_host(s, ngptot, nproma, precision, tend_planes, order, outputs, loc, seed, key, cml_before=None):
    """cloudsc_cpu_run_tendbuf_cml on the state; checks everything that does not depend on the sums: the
    inputs, BUFFER_LOC, the separate arrays and the diagnostic members keep every byte, the other kept
    outputs have the bits of cloudsc_cpu_run_precision.  Returns (cml_before, cml_after, lay)."""
    st, f, buf_tmp, buf_loc = host_set(s, ngptot, nproma, precision, tend_planes, order, outputs, loc)
    lay = cm.layout(order, tend_planes)
    nb = ca.nblocks_of(ngptot, nproma)
    buf = cm.make_buffer(nb, tend_planes, s.klev, nproma, ca.storage_dtype(precision), lay, ngptot, seed) \
        if cml_before is None else cml_before.copy()
    before, tmp_before = buf.copy(), buf_tmp.copy()
    ca.cpu_run_tendbuf_cml(ca.Params.from_dict(s.params), f, cm.bind(lay, buf), precision, outputs, ngptot, nproma,
                           s.klev, tend_planes, nthreads=3)
    assert cm.same_bits(buf_tmp, tmp_before)                                  # inputs are only read
    assert (oc.bits(buf_loc) == CANARY).all()                                 # BUFFER_LOC keeps every byte
    for n in tb.TMP + tb.LOC + tuple(oc.DIAG):
        assert (oc.bits(st.arrays[n]) == oc.SENTINEL).all(), n
    keep = ~cm.touched_mask(buf.shape, lay, ngptot)                           # vapour, other planes, padding lanes
    assert np.array_equal(tb.bits(buf)[keep], tb.bits(before)[keep])
    ref = oc.plain_run(s, key, ngptot, nproma, precision)
    for n in KEPT_OTHER:
        got, want = oc.columns(st.arrays[n], ngptot), oc.columns(ref[n], ngptot)
        if outputs == SURF and n in ca.SURFACE_FLUX_FIELDS:
            want = want[s.klev]                                               # the surface row of the profile
        assert cm.same_bits(got, want), n
    return before, buf, lay


SHAPES = [(300, 64), (300, 16), (300, 5)]
SETTINGS = [(8, "reference", PROG, "null"), (11, "permuted", SURF, "canary"), (11, "reference", PROG, "canary")]


@pytest.mark.parametrize("ngptot,nproma", SHAPES)
def test_cpu_fused_fp64_is_numpy_add_of_loc(ds, ngptot, nproma):
    for i, (planes, order, outputs, loc) in enumerate(SETTINGS):
        want_loc = oc.run_tendbuf_checked(ds, ngptot, nproma, ca.FP64, planes, order)
        before, after, lay = fused_host(ds, ngptot, nproma, ca.FP64, planes, order, outputs, loc, 7 + i, "ds")
        exp = cm.expected(before, lay, ngptot, want_loc, cm.add_storage)
        assert cm.same_bits(after, exp), (planes, order)
        m = cm.touched_mask(before.shape, lay, ngptot)
        assert np.count_nonzero(tb.bits(after)[m] != tb.bits(before)[m]) > m.sum() // 4     # the run added something


FORM_STATES = ["W", "M", "seed1", "klev3", "klev60", "klev274", "aerosol_W"]


@pytest.mark.parametrize("name", FORM_STATES)
def test_cpu_fused_fp64_on_state(ds, scenarios, name):
    s = fs.dataset(name, ds, scenarios)
    n = fs.NGPTOT
    for nproma, planes, order, outputs in ((64, 11, "permuted", PROG), (16, 8, "reference", SURF)):
        key = "forms:" + name
        want_loc = oc.run_tendbuf_checked(s, n, nproma, ca.FP64, planes, order, key)
        zero = cm.make_buffer(ca.nblocks_of(n, nproma), planes, s.klev, nproma, np.float64,
                              cm.layout(order, planes), n, 0, zero=True)
        for seed, start in ((3, None), (0, zero)):
            before, after, lay = fused_host(s, n, nproma, ca.FP64, planes, order, outputs, "null", seed, key, start)
            assert cm.same_bits(after, cm.expected(before, lay, n, want_loc, cm.add_storage)), (nproma, seed)
        if fs.rain_active(name):        # from a zero buffer: the rain plane received the rain tendency
            qr = after[:, lay["cld"] + cm.QR]
            assert np.count_nonzero(qr) > 0 and np.count_nonzero(want_loc["tendency_loc_cld"][:, cm.QR]) > 0


def widened(st):
    """The float state as doubles (ktype stays int32): exact."""
    return {n: (a if a.dtype == np.int32 else a.astype(np.float64)) for n, a in st.items()}


@pytest.mark.parametrize("name,ngptot,nproma", [("ds", 300, 64), ("ds", 300, 5), ("W", 100, 16), ("klev60", 100, 64)])
def test_cpu_fused_mixed_identity(ds, scenarios, name, ngptot, nproma):
    """out = (float) fp64_form((double) in), CML included: the mixed run on float buffers against the fp64
    run on the same values widened."""
    s = ds if name == "ds" else fs.dataset(name, ds, scenarios)
    planes, order, outputs = 11, "permuted", PROG
    lay, tlay = cm.layout(order, planes), tb.layout(order, planes)
    nb = ca.nblocks_of(ngptot, nproma)
    key = name if name == "ds" else "forms:" + name
    before32, after32, _ = fused_host(s, ngptot, nproma, ca.MIXED, planes, order, outputs, "canary", 11, key)
    # the fp64 form on the widened inputs and the widened buffer
    st32 = ca.make_host_state(s, ngptot, nproma, ca.MIXED)
    st64 = ca.HostState(ngptot, nproma, s.klev, ca.FP64, widened(st32.arrays))
    buf_tmp = tb.empty_buffer(nb, planes, s.klev, nproma, np.float64, tb.SENTINEL_TMP)
    for n in tb.TMP:
        tb.put(buf_tmp, tlay[n], st64.arrays[n], ngptot)
    m = cm.touched_mask(before32.shape, lay, ngptot)
    buf64 = np.zeros(before32.shape, dtype=np.float64)
    buf64[m] = before32[m].astype(np.float64)
    f = st64.fields()
    tb.bind(f, tlay, buf_tmp, buf_tmp)
    for n in tb.LOC + tuple(oc.DIAG):
        setattr(f, n, None)
    ca.cpu_run_tendbuf_cml(ca.Params.from_dict(s.params), f, cm.bind(lay, buf64), ca.FP64, outputs, ngptot, nproma,
                           s.klev, planes, nthreads=3)
    assert np.array_equal(tb.bits(after32)[m], tb.bits(buf64.astype(np.float32))[m])
    # and it is not the separate pass's rule: adding the narrowed float differs somewhere
    loc32 = oc.run_tendbuf_checked(s, ngptot, nproma, ca.MIXED, planes, order, key)
    unfused = cm.expected(before32, lay, ngptot, loc32, cm.add_storage)
    assert not cm.same_bits(after32, unfused)


# ---------------------------------------------------------------------------
# the separate pass
# ---------------------------------------------------------------------------
def loc_side(loc, ngptot, nproma, klev, dtype, planes):
    """tendency_loc_* as separate arrays (planes 0) or planes of a canary-backed buffer; (Fields, keepalive)."""
    f = ca.Fields()
    if not planes:
        arrays = {n: np.ascontiguousarray(loc[n]).astype(dtype) for n in tb.LOC}
        for n in tb.LOC:
            setattr(f, n, arrays[n].ctypes.data)
        return f, arrays
    nb = ca.nblocks_of(ngptot, nproma)
    lay = tb.layout("permuted", planes)
    buf = tb.empty_buffer(nb, planes, klev, nproma, dtype, CANARY)
    for n in tb.LOC:
        tb.put(buf, lay[n], np.asarray(loc[n]).astype(dtype), ngptot)
    tb.bind(f, lay, buf, buf)
    for n in tb.TMP:
        setattr(f, n, None)
    return f, buf


def cml_side(ngptot, nproma, klev, dtype, planes, seed):
    """The cumulative planes as separate arrays (planes 0: one [nb][8][klev][nproma] backing array whose
    members sit where separate arrays would: t, q, a one plane each, cld five) or a packed buffer."""
    nb = ca.nblocks_of(ngptot, nproma)
    if planes:
        lay = cm.layout("permuted", planes)
        buf = cm.make_buffer(nb, planes, klev, nproma, dtype, lay, ngptot, seed)
        return cm.bind(lay, buf), [buf], lay
    bufs, c = [], ca.TendCml()
    for k in cm.CML:
        n = ca.NCLV if k == "cld" else 1
        b = cm.make_buffer(nb, n, klev, nproma, dtype, {j: (0 if j == k else 99) for j in cm.CML}, ngptot, seed)
        setattr(c, k, b.ctypes.data)
        bufs.append(b)
    return c, bufs, None


def expected_sides(bufs, lay, ngptot, loc):
    if lay is not None:
        return [cm.expected(bufs[0], lay, ngptot, loc, cm.add_storage)]
    return [cm.expected(b, {j: (0 if j == k else 99) for j in cm.CML}, ngptot, loc, cm.add_storage)
            for k, b in zip(cm.CML, bufs)]


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED, ca.FP32], ids=["fp64", "mixed", "fp32"])
@pytest.mark.parametrize("lpl,cpl", [(0, 0), (0, 11), (11, 0), (11, 11), (8, 11)])
def test_cpu_accumulate_against_numpy(ds, precision, lpl, cpl):
    ngptot, nproma = 300, 64
    dt = ca.storage_dtype(precision)
    loc = oc.run_tendbuf_checked(ds, ngptot, nproma, ca.FP64, 8, "reference")       # any real tendencies
    loc = {n: np.asarray(loc[n]).astype(dt) for n in tb.LOC}
    f, keep = loc_side(loc, ngptot, nproma, ds.klev, dt, lpl)
    c, bufs, lay = cml_side(ngptot, nproma, ds.klev, dt, cpl, 21)
    want = expected_sides(bufs, lay, ngptot, loc)
    src_before = keep.copy() if lpl else None
    for nthreads in (1, 3):
        work = [b.copy() for b in bufs]
        c2 = cm.bind(lay, work[0]) if lay is not None else ca.TendCml(*[w.ctypes.data for w in work])
        ca.cpu_accumulate_tendbuf(f, c2, precision, ngptot, nproma, ds.klev, lpl, cpl, nthreads=nthreads)
        for w, e in zip(work, want):
            assert cm.same_bits(w, e), (lpl, cpl, nthreads)
    if lpl:
        assert cm.same_bits(keep, src_before)                                      # the source is only read
    del c


@pytest.mark.parametrize("ngptot,nproma", [(300, 64), (300, 5)])
def test_cpu_fused_fp64_is_step_plus_pass(ds, ngptot, nproma):
    planes, order = 11, "permuted"
    before, fused, lay = fused_host(ds, ngptot, nproma, ca.FP64, planes, order, PROG, "null", 5, "ds")
    loc = oc.run_tendbuf_checked(ds, ngptot, nproma, ca.FP64, planes, order)
    f, keep = loc_side(loc, ngptot, nproma, ds.klev, np.float64, planes)
    two = before.copy()
    ca.cpu_accumulate_tendbuf(f, cm.bind(lay, two), ca.FP64, ngptot, nproma, ds.klev, planes, planes, nthreads=2)
    assert cm.same_bits(two, fused)
    # a launch adds once; a second one accumulates again
    ca.cpu_accumulate_tendbuf(f, cm.bind(lay, two), ca.FP64, ngptot, nproma, ds.klev, planes, planes, nthreads=2)
    assert cm.same_bits(two, cm.expected(fused, lay, ngptot, loc, cm.add_storage))


@pytest.mark.parametrize("extra,word", [
    ([], "--fields tendbuf-cml needs --outputs prognostic|surface"),
    (["--outputs", "all"], "--fields tendbuf-cml needs --outputs prognostic|surface"),
    (["--outputs", "prognostic", "--variant", "scc"], "--outputs goes with"),
])
def test_cli_tendbuf_cml_refusals(extra, word):
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    r = subprocess.run([exe, "1", "300", "64", "--fields", "tendbuf-cml"] + extra, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and word in r.stderr, r.stderr
