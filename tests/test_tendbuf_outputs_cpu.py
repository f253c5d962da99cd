"""The prognostic step and the in-place checks on packed tendency buffers, without a GPU: every argument
rule of the seven entry points, the ALL / 0-plane degenerate cases against the existing entry points,
cloudsc_cpu_run_tendbuf_outputs(PROGNOSTIC) against cloudsc_cpu_run_precision on separate arrays and the fp64
oracle (also on the 23 states of tests/form_state_cases.py), and cloudsc_cpu_fields_compare_tendbuf against
the NumPy restatement of tests/fields_compare_cases.py on whole buffers -- all on raw bits, the buffers
pre-filled with sentinel bytes that unbound planes and padding lanes must keep."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import fields_compare_cases as cc
import fields_convert_cases as fc
import form_state_cases as fs
import tendbuf_cases as tb
import host_harness as oc
from host_harness import KLEV, PackedSide, cpu_compare

DIAG, KEPT = oc.DIAG, oc.KEPT
SHAPES = list(tb.SHAPES) + [(1, 1)]
SETTINGS = [(8, "reference"), (11, "permuted")]
PROG, ALL = ca.OUTPUTS_PROGNOSTIC, ca.OUTPUTS_ALL


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


def ref_of(p):
    return C.byref(p) if p is not None else None


# ---------------------------------------------------------------------------
# argument rules: each returns its code on a machine without a GPU
# ---------------------------------------------------------------------------
def test_gpu_run_tendbuf_outputs_rules_need_no_gpu(lib):
    f = oc.full_fields()
    ws = C.c_void_p(0x10)

    def run(prec=ca.FP64, variant=ca.VARIANT_KSEG, outputs=PROG, ngptot=100, nproma=16, klev=KLEV, planes=8, fields=f,
            scratch=ws):
        return lib.cloudsc_gpu_run_tendbuf_outputs(0, None, prec, variant, outputs, ngptot, nproma, klev, planes,
                                                   ref_of(fields), scratch)
    for outputs in (2, -1, 99):
        assert run(outputs=outputs) == ca.EINVAL
    for outputs in (ALL, PROG):
        for planes in (7, 65, 0, -1):
            assert run(outputs=outputs, planes=planes) == ca.EINVAL
        for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, 77, ca.VARIANT_KSEG | 0x1000,
                        ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM, ca.VARIANT_KCACHE | ca.FP32_EXACT_LIBM):
            assert run(outputs=outputs, variant=variant) == ca.EINVAL
            assert run(outputs=outputs, prec=ca.FP32, variant=variant) == ca.EINVAL
        assert run(outputs=outputs, prec=99) == ca.EINVAL
        assert run(outputs=outputs, ngptot=0) == ca.EINVAL
        assert run(outputs=outputs, nproma=0) == ca.EINVAL
        assert run(outputs=outputs, klev=1) == ca.EINVAL
        assert run(outputs=outputs, variant=ca.VARIANT_KCACHE, nproma=257) == ca.EINVAL
        assert run(outputs=outputs, fields=None) == ca.EINVAL
        assert run(outputs=outputs, scratch=None) == ca.EINVAL               # KSEG needs its workspace
        for missing in KEPT + ("pt", "tendency_tmp_cld", "ktype"):           # a kept output or an input missing
            assert run(outputs=outputs, fields=oc.full_fields(without=(missing,))) == ca.EINVAL, missing
    assert run(outputs=ALL, fields=oc.full_fields(without=("pfsqlf",))) == ca.EINVAL   # ALL needs all 21


def test_gpu_run_tendbuf_outputs_all_is_gpu_run_tendbuf(lib):
    """Calls that can never launch: the same code as cloudsc_gpu_run_tendbuf."""
    ws = C.c_void_p(0x10)
    f = oc.full_fields()
    cases = [dict(planes=7), dict(prec=99), dict(variant=77), dict(variant=ca.VARIANT_SCC), dict(ngptot=0),
             dict(nproma=0), dict(klev=1), dict(fields=None), dict(fields=oc.full_fields(without=DIAG)),
             dict(variant=ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM)]
    for kw in cases:
        a = dict(prec=ca.FP64, variant=ca.VARIANT_KSEG, ngptot=100, nproma=16, klev=KLEV, planes=8, fields=f)
        a.update(kw)
        fp = ref_of(a["fields"])
        want = lib.cloudsc_gpu_run_tendbuf(0, None, a["prec"], a["variant"], a["ngptot"], a["nproma"], a["klev"],
                                           a["planes"], fp, ws)
        got = lib.cloudsc_gpu_run_tendbuf_outputs(0, None, a["prec"], a["variant"], ALL, a["ngptot"], a["nproma"],
                                                  a["klev"], a["planes"], fp, ws)
        assert got == want and got != 0, kw


def test_cpu_run_tendbuf_outputs_rules(lib, ds):
    f = oc.full_fields()
    p = ca.Params.from_dict(ds.params)

    def run(prec=ca.FP64, outputs=PROG, ngptot=100, nproma=16, klev=KLEV, planes=8, params=p, fields=f):
        return lib.cloudsc_cpu_run_tendbuf_outputs(1, prec, outputs, ngptot, nproma, klev, planes, ref_of(params),
                                                   ref_of(fields))
    for outputs in (2, -1, 99):
        assert run(outputs=outputs) == ca.EINVAL
    for outputs in (ALL, PROG):
        for planes in (7, 65, 0, -1):
            assert run(outputs=outputs, planes=planes) == ca.EINVAL
        assert run(outputs=outputs, prec=ca.FP32) == ca.EINVAL   # the fp32 arithmetic has no host form
        assert run(outputs=outputs, prec=99) == ca.EINVAL
        assert run(outputs=outputs, ngptot=0) == ca.EINVAL
        assert run(outputs=outputs, nproma=0) == ca.EINVAL
        assert run(outputs=outputs, klev=1) == ca.EINVAL
        assert run(outputs=outputs, params=None) == ca.EINVAL
        assert run(outputs=outputs, fields=None) == ca.EINVAL
        for missing in KEPT + ("tendency_tmp_t",):
            assert run(outputs=outputs, fields=oc.full_fields(without=(missing,))) == ca.EINVAL, missing
    assert run(outputs=ALL, fields=oc.full_fields(without=("pfsqitur",))) == ca.EINVAL


@pytest.mark.parametrize("device_form", [False, True])
def test_compare_tendbuf_rules_need_no_gpu(lib, device_form):
    a, b = ca.Fields(), ca.Fields()
    a.pt, b.pt = 0x1000, 0x2000
    a.tendency_loc_t, b.tendency_loc_t = 0x3000, 0x4000
    diffs = cc.new_diffs()

    def cmp(ngptot=100, klev=3, ap=ca.FP64, anp=16, apl=8, fa=a, bp=ca.FP64, bnp=16, bpl=0, fb=b, d=diffs):
        if device_form:
            return lib.cloudsc_fields_compare_tendbuf(0, None, ngptot, klev, ap, anp, apl, ref_of(fa), bp, bnp, bpl,
                                                      ref_of(fb), d)
        return lib.cloudsc_cpu_fields_compare_tendbuf(1, ngptot, klev, ap, anp, apl, ref_of(fa), bp, bnp, bpl,
                                                      ref_of(fb), d)
    for planes in (7, 65, -1, 1):
        assert cmp(apl=planes) == ca.EINVAL
        assert cmp(bpl=planes) == ca.EINVAL
    for apl, bpl in ((8, 0), (0, 11), (8, 11), (0, 0)):
        kw = dict(apl=apl, bpl=bpl)
        assert cmp(fa=None, **kw) == ca.EINVAL
        assert cmp(fb=None, **kw) == ca.EINVAL
        assert cmp(d=None, **kw) == ca.EINVAL
        assert cmp(ap=99, **kw) == ca.EINVAL
        assert cmp(bp=99, **kw) == ca.EINVAL
        assert cmp(ngptot=0, **kw) == ca.EINVAL
        assert cmp(klev=0, **kw) == ca.EINVAL
        assert cmp(anp=0, **kw) == ca.EINVAL
        assert cmp(bnp=(1 << 24) + 1, **kw) == ca.EINVAL
        assert cmp(fa=ca.Fields(), fb=ca.Fields(), **kw) == ca.EINVAL      # nothing to compare
        c = ca.Fields()
        c.pt = 0x2000
        assert cmp(fb=c, **kw) == ca.EINVAL                                # a member set on one side only


def reference_struct(klev, klon=100, without=()):
    """A Reference whose arrays are never read (the calls fail first); ids in `without` are NULL."""
    r = ca.Reference()
    r.klon, r.klev = klon, klev
    for i in range(len(ca.VALIDATED)):
        r.field[i] = None if i in without else 0x100000 + 0x1000 * i
    return r


def test_validate_tendbuf_rules_need_no_gpu(lib):
    names = [k for _, k in ca.VALIDATED]
    diag_ids = [i for i, k in enumerate(names) if k in DIAG]
    kept_ids = [i for i, k in enumerate(names) if k in KEPT]
    assert len(diag_ids) == 10 and len(kept_ids) == 11
    f, r = oc.full_fields(), reference_struct(KLEV)
    stats = (ca.Stats * len(names))()

    def val(prec=ca.FP64, ngptot=100, nproma=16, klev=KLEV, planes=8, outputs=PROG, off=0, fields=f, ref=r, st=stats):
        return lib.cloudsc_fields_validate_tendbuf(0, None, prec, ngptot, nproma, klev, planes, outputs, off,
                                                   ref_of(fields), ref_of(ref), st)
    for planes in (7, 65, -1, 1):
        assert val(planes=planes) == ca.EINVAL
    for outputs in (2, -1, 99):
        assert val(outputs=outputs) == ca.EINVAL
    for outputs, planes in ((ALL, 0), (ALL, 8), (PROG, 0), (PROG, 11)):
        kw = dict(outputs=outputs, planes=planes)
        assert val(fields=None, **kw) == ca.EINVAL
        assert val(ref=None, **kw) == ca.EINVAL
        assert val(st=None, **kw) == ca.EINVAL
        assert val(prec=99, **kw) == ca.EINVAL
        assert val(ngptot=0, **kw) == ca.EINVAL
        assert val(nproma=0, **kw) == ca.EINVAL
        assert val(nproma=(1 << 24) + 1, **kw) == ca.EINVAL
        assert val(klev=0, **kw) == ca.EINVAL
        assert val(off=-1, **kw) == ca.EINVAL
        assert val(ref=reference_struct(KLEV + 1), **kw) == ca.EINVAL
        assert val(ref=reference_struct(KLEV, klon=0), **kw) == ca.EINVAL
        for i in kept_ids:                                  # a kept member / its reference array missing
            assert val(fields=oc.full_fields(without=(names[i],)), **kw) == ca.EINVAL, names[i]
            assert val(ref=reference_struct(KLEV, without=(i,)), **kw) == ca.EINVAL, names[i]
        for i in diag_ids:                                  # a diagnostic member on one side only
            assert val(fields=oc.full_fields(without=(names[i],)), **kw) == ca.EINVAL, names[i]
            assert val(ref=reference_struct(KLEV, without=(i,)), **kw) == ca.EINVAL, names[i]
    # ALL needs all 21 on both sides, also when both are absent
    assert val(outputs=ALL, fields=oc.full_fields(without=DIAG), ref=reference_struct(KLEV, without=diag_ids)) == ca.EINVAL
    # what is left is a well-formed call: without a device it gets as far as asking for one
    rc = val(outputs=PROG, fields=oc.full_fields(without=DIAG), ref=reference_struct(KLEV, without=diag_ids))
    assert rc != ca.EINVAL and (rc != 0 or ca.device_count() > 0)


def test_expand_tendbuf_rules_need_no_gpu(lib, ds):
    t = ca.make_template(ds, [])
    f = ca.Fields()
    f.pt, f.tendency_tmp_t = 0x1000, 0x2000

    def exp(prec=ca.FP64, ngptot=100, nproma=16, planes=8, off=0, tmpl=t, fields=f):
        return lib.cloudsc_fields_expand_tendbuf(0, None, prec, ngptot, nproma, planes, off, ref_of(tmpl),
                                                 ref_of(fields))
    for planes in (7, 65, 0, -1):
        assert exp(planes=planes) == ca.EINVAL
    assert exp(tmpl=None) == ca.EINVAL
    assert exp(fields=None) == ca.EINVAL
    assert exp(prec=99) == ca.EINVAL
    assert exp(ngptot=0) == ca.EINVAL
    assert exp(nproma=0) == ca.EINVAL
    assert exp(nproma=(1 << 24) + 1) == ca.EINVAL
    assert exp(off=-1) == ca.EINVAL
    assert exp(fields=ca.Fields()) == ca.EINVAL                 # nothing to fill
    g = ca.Fields()
    g.tendency_loc_t = 0x3000                                   # outputs are not filled: nothing to fill
    assert exp(fields=g) == ca.EINVAL


OUTPUTS_GOES_WITH = "--outputs goes with --fields caller|tendbuf|tendbuf-inplace"
TENDBUF_RUNS = "--fields tendbuf runs --variant kseg|kcache"


@pytest.mark.parametrize("extra,word", [
    (["--outputs", "prognostic"], OUTPUTS_GOES_WITH),
    (["--fields", "state", "--outputs", "prognostic"], OUTPUTS_GOES_WITH),
    (["--fields", "caller", "--outputs", "prognostic", "--variant", "scc"], OUTPUTS_GOES_WITH),
    (["--fields", "caller", "--outputs", "prognostic", "--transfer"], OUTPUTS_GOES_WITH),
    (["--fields", "caller", "--outputs", "prognostic", "--fp32-exact-libm"], OUTPUTS_GOES_WITH),
    (["--fields", "caller", "--outputs", "some"], "bad --outputs some"),
    (["--fields", "tendbuf-inplace", "--variant", "scc"], TENDBUF_RUNS),
    (["--fields", "tendbuf-inplace", "--variant", "cpu"], TENDBUF_RUNS),
    (["--fields", "tendbuf-inplace", "--transfer"], TENDBUF_RUNS),
    (["--fields", "tendbuf-inplace", "--fp32-exact-libm"], "--fields tendbuf-inplace has no --fp32-exact-libm form"),
    (["--fields", "tendbuf-inplace", "--tend-planes", "7"], "bad --tend-planes 7"),
])
def test_cli_refusals(extra, word):
    """The messages of the new checks, not the "unknown option" / "bad --fields" a CLI without them prints."""
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    r = subprocess.run([exe, "1", "300", "64"] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and word in r.stderr, r.stderr


# ---------------------------------------------------------------------------
# cloudsc_cpu_run_tendbuf_outputs
# ---------------------------------------------------------------------------
def run_form(s, ngptot, nproma, precision, tend_planes, order, outputs, diag, key):
    """cloudsc_cpu_run_tendbuf_outputs on the dataset, checked for the sentinels and against
    cloudsc_cpu_run_precision on separate arrays; diag: the ten diagnostic members "null" or "sentinel".
    Returns {name: block-layout array}."""
    ref = oc.plain_run(s, key, ngptot, nproma, precision)
    st = ca.make_host_state(s, ngptot, nproma, precision)
    nb, dt = ca.nblocks_of(ngptot, nproma), ca.storage_dtype(precision)
    lay = tb.layout(order, tend_planes)
    buf_tmp = tb.empty_buffer(nb, tend_planes, s.klev, nproma, dt, tb.SENTINEL_TMP)
    buf_loc = tb.empty_buffer(nb, tend_planes, s.klev, nproma, dt, tb.SENTINEL_LOC)
    for n in tb.TMP:
        tb.put(buf_tmp, lay[n], st.arrays[n], ngptot)
    tmp_before = buf_tmp.copy()
    for n in DIAG:
        st.arrays[n].view(np.uint8)[...] = oc.SENTINEL
    for n in tb.TMP + tb.LOC:                          # the separate tendency arrays are not the run's
        st.arrays[n].view(np.uint8)[...] = oc.SENTINEL
    f = st.fields()
    if order == "reference":
        ca.bind_tendbuf(f, precision, nproma, s.klev, buf_tmp.ctypes.data, buf_loc.ctypes.data)
    else:
        tb.bind(f, lay, buf_tmp, buf_loc)
    if diag == "null":
        for n in DIAG:
            setattr(f, n, None)
    ca.cpu_run_tendbuf_outputs(ca.Params.from_dict(s.params), f, precision, outputs, ngptot, nproma, s.klev,
                               tend_planes, nthreads=3)
    assert np.array_equal(tb.bits(buf_tmp), tb.bits(tmp_before))            # inputs are only read
    assert tb.is_sentinel(buf_loc, tb.untouched_mask(buf_loc, lay, tb.LOC, ngptot), tb.SENTINEL_LOC)
    for n in tb.TMP + tb.LOC:
        assert (oc.bits(st.arrays[n]) == oc.SENTINEL).all(), n
    if outputs == PROG:
        for n in DIAG:
            assert (oc.bits(st.arrays[n]) == oc.SENTINEL).all(), n
    got = {k: tb.take(buf_loc, lay[k], k) if k in tb.LOC else st.arrays[k] for k in oc.ALL21}
    names = KEPT if outputs == PROG else oc.ALL21
    assert [k for k in names
            if not np.array_equal(tb.bits(oc.columns(got[k], ngptot)), tb.bits(oc.columns(ref[k], ngptot)))] == []
    return got


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED], ids=["fp64", "mixed"])
@pytest.mark.parametrize("ngptot,nproma", SHAPES)
def test_cpu_run_tendbuf_outputs_prognostic(ds, oracle_mod, ngptot, nproma, precision):
    for tend_planes, order in SETTINGS:
        for diag in ("null", "sentinel"):
            got = run_form(ds, ngptot, nproma, precision, tend_planes, order, PROG, diag, "ds")
            if precision == ca.FP64:
                ost, _ = oracle_mod.run_oracle(ds, ngptot, nproma)
                for k in KEPT:
                    assert np.array_equal(tb.bits(oc.columns(got[k], ngptot)),
                                          tb.bits(oc.columns(ost.arrays[k], ngptot))), (k, tend_planes, diag)


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED], ids=["fp64", "mixed"])
def test_cpu_run_tendbuf_outputs_all_is_cpu_run_tendbuf(ds, precision):
    """OUTPUTS_ALL: the bits of cloudsc_cpu_run_tendbuf, all 21 fields (the diagnostic ones written)."""
    for ngptot, nproma in ((300, 64), (100, 16)):
        want = oc.run_tendbuf_checked(ds, ngptot, nproma, precision, 11, "permuted")
        got = run_form(ds, ngptot, nproma, precision, 11, "permuted", ALL, "sentinel", "ds")
        for k in oc.ALL21:
            assert np.array_equal(tb.bits(oc.columns(got[k], ngptot)), tb.bits(oc.columns(want[k], ngptot))), k


@pytest.mark.parametrize("name", fs.STATES)
def test_cpu_tendbuf_prognostic_on_state(ds, scenarios, oracle_mod, name):
    s = fs.dataset(name, ds, scenarios)
    exp = fs.oracle_outputs(oracle_mod, name, s)
    n = fs.NGPTOT
    for nproma in (64, 16):
        got = run_form(s, n, nproma, ca.FP64, 11, "permuted", PROG, "null", "forms:" + name)
        assert [k for k in KEPT if not np.array_equal(tb.bits(oc.columns(got[k], n)), tb.bits(exp[k]))] == [], nproma
        if fs.rain_active(name):        # the carried rain flux reached its output
            assert np.count_nonzero(oc.columns(got["pfplsl"], n)) > 0, nproma


# ---------------------------------------------------------------------------
# cloudsc_cpu_fields_compare_tendbuf against NumPy on whole buffers
# ---------------------------------------------------------------------------
# (planes, NPROMA, precision) of a side
SIDES = [(pl, np_, pr) for pl in (0, 8, 11) for np_ in (64, 16) for pr in (ca.FP64, ca.MIXED)]


@pytest.mark.parametrize("klev,ngptot", [(3, 300), (137, 150)])
def test_cpu_compare_tendbuf_equal_sets_every_pairing(klev, ngptot):
    names = list(tb.TMP + tb.LOC) + ["pt", "pfplsl", "ktype", "prainfrac_toprfz"]
    for apl, anp, apr in SIDES:
        for bpl, bnp, bpr in SIDES:
            if klev == 137 and (anp, apr) == (bnp, bpr) and apl == bpl:
                continue
            ha, hb, _ = cc.make_pair(ngptot, anp, bnp, klev, apr, bpr, names=names, plant=False)
            a, b = PackedSide(ha, apl), PackedSide(hb, bpl, "reference" if bpl == 8 else "permuted")
            diffs = cpu_compare(a, b)
            cc.check_against_restatement(diffs, cc.restate(a.view(), b.view()))
            assert sum(d.mismatches for d in diffs) == 0, (apl, anp, apr, bpl, bnp, bpr)
            assert sum(1 for d in diffs if d.compared) == len(names)


@pytest.mark.parametrize("apl,bpl", [(8, 0), (0, 11), (11, 8), (0, 0)])
def test_cpu_compare_tendbuf_planted_against_numpy(apl, bpl):
    """Every member, planted differences (the last active lane of the partial last block among them)."""
    ha, hb, pos = cc.make_pair(300, 64, 16, 3, ca.FP64, ca.MIXED)
    a, b = PackedSide(ha, apl), PackedSide(hb, bpl)
    diffs = cpu_compare(a, b)
    exp = cc.restate(a.view(), b.view())
    assert sum(e["mismatches"] for e in exp.values()) >= len(set(pos))
    cc.check_against_restatement(diffs, exp)
    if not apl and not bpl:             # 0 and 0 is cloudsc_cpu_fields_compare, bit for bit
        plain = cc.new_diffs()
        ca.check(ca.gpu_lib().cloudsc_cpu_fields_compare(3, 300, 3, ca.FP64, 64, C.byref(a.f), ca.MIXED, 16,
                                                         C.byref(b.f), plain))
        assert bytes(plain) == bytes(diffs)


@pytest.mark.parametrize("ngptot,nproma", [(300, 300), (1, 1)])
def test_cpu_compare_tendbuf_one_block(ngptot, nproma):
    """One block on both sides: the block stride is never used (a build that takes the member's own rows for
    it passes here and fails every case above with two or more blocks)."""
    ha, hb, pos = cc.make_pair(ngptot, nproma, nproma, 3, ca.FP64, ca.MIXED)
    a, b = PackedSide(ha, 11), PackedSide(hb, 8, "reference")
    diffs = cpu_compare(a, b)
    exp = cc.restate(a.view(), b.view())
    assert sum(e["mismatches"] for e in exp.values()) >= 1
    cc.check_against_restatement(diffs, exp)


def test_cpu_compare_tendbuf_bit_flip_found_unbound_and_padding_ignored():
    ngptot, anp, bnp, klev = 300, 64, 16, 137
    names = list(tb.TMP + tb.LOC) + ["pt"]
    ha, hb, _ = cc.make_pair(ngptot, anp, bnp, klev, ca.FP64, ca.FP64, names=names, plant=False)
    a, b = PackedSide(ha, 11), PackedSide(hb, 8, "reference")
    buf, lay = a.bufs[1], a.lay
    nb = buf.shape[0]
    tail = ngptot - (nb - 1) * anp
    assert 0 < tail < anp
    bound = set()
    for n in tb.LOC:
        bound |= set(range(lay[n], lay[n] + tb.nplanes(n)))
    unbound = sorted(set(range(11)) - bound)
    assert len(unbound) == 3
    tb.bits(buf)[nb - 1, unbound[0], 5, 1] ^= 1                     # an unbound plane
    tb.bits(buf)[nb - 1, lay["tendency_loc_q"], 7, tail] ^= 1       # a padding lane of a bound plane
    tb.bits(a.bufs[0])[0, sorted(set(range(11)) - {lay[n] + i for n in tb.TMP for i in range(tb.nplanes(n))})[0], 0,
                       0] ^= 1
    assert sum(d.mismatches for d in cpu_compare(a, b)) == 0
    # one bit in tendency_loc_cld, species 2, level 100, the last real column of the partial block
    row, col = 2 * klev + 100, ngptot - 1
    tb.bits(buf)[nb - 1, lay["tendency_loc_cld"] + 2, 100, tail - 1] ^= 1 << 20
    for nthreads in (1, 3):
        diffs = cpu_compare(a, b, nthreads)
        hit = {fc.MEMBERS[m]: (d.mismatches, d.first_column, d.first_row) for m, d in enumerate(diffs) if d.mismatches}
        assert hit == {"tendency_loc_cld": (1, col, row)}
        cc.check_against_restatement(diffs, cc.restate(a.view(), b.view()))
