"""Packed tendency buffers without a GPU: the argument rules of the five entry
points, cloudsc_cpu_run_tendbuf against cloudsc_cpu_run_precision on the same
values in separate arrays (and the fp64 oracle), and
cloudsc_cpu_fields_convert_tendbuf against a NumPy restatement -- all on raw
bits, with the buffers pre-filled with sentinel bytes that unbound planes and
padding lanes must keep."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import fields_convert_cases as fc
import tendbuf_cases as tb
from host_harness import CONV_CASES, CONV_KLEV, CONV_NGPTOT, KLEV, NAMES, Side, columns, convert, full_fields
from host_harness import run_tendbuf_checked, same_storage


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


# ---------------------------------------------------------------------------
# argument rules
# ---------------------------------------------------------------------------
def test_bind_rules_and_planes(lib):
    f = ca.Fields()
    bad = [(None, ca.FP64, 16, 5, 64, 128), (f, 99, 16, 5, 64, 128), (f, ca.FP64, 0, 5, 64, 128),
           (f, ca.FP64, 16, 0, 64, 128), (f, ca.FP64, 16, 5, None, 128), (f, ca.FP64, 16, 5, 64, None)]
    for fields, prec, nproma, klev, t, l in bad:
        assert lib.cloudsc_tendbuf_bind(C.byref(fields) if fields is not None else None, prec, nproma, klev, t,
                                        l) == ca.EINVAL
    for prec, es in ((ca.FP64, 8), (ca.MIXED, 4), (ca.FP32, 4)):
        f = ca.Fields()
        ca.bind_tendbuf(f, prec, 16, 5, 1 << 20, 1 << 24)
        plane = 16 * 5 * es
        want = {"t": ca.TENDBUF_T, "a": ca.TENDBUF_A, "q": ca.TENDBUF_Q, "cld": ca.TENDBUF_CLD}
        assert (ca.TENDBUF_T, ca.TENDBUF_A, ca.TENDBUF_Q, ca.TENDBUF_CLD) == (0, 1, 2, 3)
        for k, p in want.items():
            assert getattr(f, "tendency_tmp_" + k) == (1 << 20) + p * plane
            assert getattr(f, "tendency_loc_" + k) == (1 << 24) + p * plane
        assert not f.pt and not f.plude


def test_gpu_run_tendbuf_rules_need_no_gpu(lib):
    f = full_fields()
    ws = C.c_void_p(0x10)

    def run(prec=ca.FP64, variant=ca.VARIANT_KSEG, ngptot=100, nproma=16, klev=KLEV, planes=8, fields=f, scratch=ws):
        return lib.cloudsc_gpu_run_tendbuf(0, None, prec, variant, ngptot, nproma, klev, planes,
                                           C.byref(fields) if fields is not None else None, scratch)
    for planes in (7, 65, 0, -1):
        assert run(planes=planes) == ca.EINVAL
    for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, 77, ca.VARIANT_KSEG | 0x1000,
                    ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM):
        assert run(variant=variant) == ca.EINVAL
    assert run(prec=99) == ca.EINVAL
    assert run(ngptot=0) == ca.EINVAL
    assert run(nproma=0) == ca.EINVAL
    assert run(klev=1) == ca.EINVAL
    assert run(variant=ca.VARIANT_KCACHE, nproma=257) == ca.EINVAL
    assert run(fields=None) == ca.EINVAL
    assert run(scratch=None) == ca.EINVAL               # KSEG needs its workspace
    g = full_fields()
    g.tendency_loc_cld = None
    assert run(fields=g) == ca.EINVAL


def test_cpu_run_tendbuf_rules(lib, ds):
    f = full_fields()
    p = ca.Params.from_dict(ds.params)

    def run(prec=ca.FP64, ngptot=100, nproma=16, klev=KLEV, planes=8, params=p, fields=f):
        return lib.cloudsc_cpu_run_tendbuf(1, prec, ngptot, nproma, klev, planes,
                                           C.byref(params) if params is not None else None,
                                           C.byref(fields) if fields is not None else None)
    for planes in (7, 65, 0, -1):
        assert run(planes=planes) == ca.EINVAL
    assert run(prec=ca.FP32) == ca.EINVAL               # the fp32 arithmetic has no host form
    assert run(prec=99) == ca.EINVAL
    assert run(ngptot=0) == ca.EINVAL
    assert run(nproma=0) == ca.EINVAL
    assert run(klev=1) == ca.EINVAL
    assert run(params=None) == ca.EINVAL
    assert run(fields=None) == ca.EINVAL
    g = full_fields()
    g.tendency_tmp_t = None
    assert run(fields=g) == ca.EINVAL


@pytest.mark.parametrize("device_form", [False, True])
def test_convert_tendbuf_rules_need_no_gpu(lib, device_form):
    a, b = ca.Fields(), ca.Fields()
    a.pt, b.pt = 0x1000, 0x2000
    a.tendency_tmp_t, b.tendency_tmp_t = 0x3000, 0x4000

    def conv(ngptot=100, klev=3, sp=ca.FP64, snp=16, spl=8, src=a, dp=ca.FP64, dnp=16, dpl=0, dst=b):
        s = C.byref(src) if src is not None else None
        d = C.byref(dst) if dst is not None else None
        if device_form:
            return lib.cloudsc_fields_convert_tendbuf(0, None, ngptot, klev, sp, snp, spl, s, dp, dnp, dpl, d)
        return lib.cloudsc_cpu_fields_convert_tendbuf(1, ngptot, klev, sp, snp, spl, s, dp, dnp, dpl, d)
    for planes in (7, 65, -1, 1):
        assert conv(spl=planes) == ca.EINVAL
        assert conv(dpl=planes) == ca.EINVAL
    assert conv(src=None) == ca.EINVAL
    assert conv(dst=None) == ca.EINVAL
    assert conv(sp=99) == ca.EINVAL
    assert conv(dp=99) == ca.EINVAL
    assert conv(ngptot=0) == ca.EINVAL
    assert conv(klev=0) == ca.EINVAL
    assert conv(snp=0) == ca.EINVAL
    assert conv(dnp=(1 << 24) + 1) == ca.EINVAL
    assert conv(src=ca.Fields(), dst=ca.Fields()) == ca.EINVAL      # nothing to convert
    c = ca.Fields()
    c.pt = 0x2000
    assert conv(dst=c) == ca.EINVAL                                 # a member set on one side only
    c.tendency_tmp_t = 0x3000
    assert conv(dst=c) == ca.EINVAL                                 # the same array on both sides


@pytest.mark.parametrize("extra", [["--transfer"], ["--variant", "cpu"], ["--variant", "scc"],
                                   ["--variant", "scc-private"]], ids=["transfer", "cpu", "scc", "scc-private"])
def test_cli_fields_tendbuf_refusals(extra):
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    r = subprocess.run([exe, "1", "300", "64", "--fields", "tendbuf"] + extra, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--fields tendbuf" in r.stderr
    r = subprocess.run([exe, "1", "300", "64", "--fields", "tendbuf", "--tend-planes", "7"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode != 0 and "--tend-planes" in r.stderr


# ---------------------------------------------------------------------------
# cloudsc_cpu_run_tendbuf
# ---------------------------------------------------------------------------
CPU_SHAPES = list(tb.SHAPES)


@pytest.mark.parametrize("order", ["reference", "permuted"])
@pytest.mark.parametrize("tend_planes", [8, 11])
@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED])
@pytest.mark.parametrize("ngptot,nproma", CPU_SHAPES)
def test_cpu_run_tendbuf_bitwise(ds, oracle_mod, ngptot, nproma, precision, tend_planes, order):
    got = run_tendbuf_checked(ds, ngptot, nproma, precision, tend_planes, order)
    if precision == ca.FP64:
        ost, _ = oracle_mod.run_oracle(ds, ngptot, nproma)
        for k in NAMES:
            assert np.array_equal(tb.bits(columns(got[k], ngptot)), tb.bits(columns(ost.arrays[k], ngptot))), k


# ---------------------------------------------------------------------------
# cloudsc_cpu_fields_convert_tendbuf against NumPy
# ---------------------------------------------------------------------------
def expected_after(src, dst):
    """dst's storage after the conversion, restated: every valid lane the cast value, the rest as before."""
    out = dst.snapshot()
    names = list(dst.arrays)
    for i, name in enumerate(names):
        dt = fc.dtype_of(name, dst.precision)
        vals = columns(src.member(name), src.ngptot).astype(dt)       # [rows..][ngptot]
        blocks = fc.to_blocks(vals.reshape(-1, src.ngptot), dst.nproma, dt, 0).reshape(dst.arrays[name].shape)
        packed = dst.tend_planes and name in tb.TMP + tb.LOC
        if packed:
            buf = out[len(names) + (0 if name in tb.TMP else 1)]
            tb.put(buf, dst.lay[name], blocks, dst.ngptot)
        else:
            for b in range(dst.nb):
                n = min(dst.nproma, dst.ngptot - b * dst.nproma)
                out[i][b, ..., :n] = blocks[b, ..., :n]
    return out


@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_cpu_convert_tendbuf_against_numpy(case):
    s, d = CONV_CASES[case]
    src, dst = Side(*s), Side(*d, values=False)
    before = src.snapshot()
    want = expected_after(src, dst)
    convert(src, dst)
    assert same_storage(src.snapshot(), before)
    assert same_storage(dst.snapshot(), want)
    # the restatement itself moved something into the buffers, and left sentinels where it should
    if dst.tend_planes:
        assert tb.is_sentinel(dst.bufs[1], tb.untouched_mask(dst.bufs[1], dst.lay, tb.LOC, dst.ngptot), tb.SENTINEL_LOC)
        assert not tb.is_sentinel(dst.bufs[1], ~tb.untouched_mask(dst.bufs[1], dst.lay, tb.LOC, dst.ngptot),
                                  tb.SENTINEL_LOC)


def test_cpu_convert_tendbuf_round_trip():
    src = Side(ca.FP64, 24, 0)
    mid = Side(ca.FP64, 64, 11, "permuted", values=False)
    back = Side(ca.FP64, 24, 0, values=False)
    convert(src, mid)
    convert(mid, back)
    for name in fc.MEMBERS:
        assert np.array_equal(tb.bits(columns(back.arrays[name], CONV_NGPTOT)),
                              tb.bits(columns(src.arrays[name], CONV_NGPTOT))), name


def test_cpu_convert_tendbuf_zero_planes_is_convert():
    src = Side(ca.FP64, 24, 0)
    a, b = Side(ca.MIXED, 64, 0, values=False), Side(ca.MIXED, 64, 0, values=False)
    convert(src, a)
    ca.check(ca.gpu_lib().cloudsc_cpu_fields_convert(3, CONV_NGPTOT, CONV_KLEV, src.precision, src.nproma,
                                                     C.byref(src.f), b.precision, b.nproma, C.byref(b.f)))
    assert same_storage(a.snapshot(), b.snapshot())
    assert not tb.is_sentinel(a.arrays["pt"], np.ones(a.arrays["pt"].shape, bool), tb.SENTINEL_LOC)
