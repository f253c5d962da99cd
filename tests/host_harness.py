"""TEST INFRASTRUCTURE ONLY -- what several test files need on the host, once: bit views and columns, the host
runs the forms are compared with (cloudsc_cpu_run_precision, cloudsc_cpu_run_outputs, cloudsc_cpu_run_tendbuf),
the host sides of the tendency-buffer conversions and comparisons, the configured datasets, the argument rules
of cloudsc_gpu_run_spp, and the reference harness's stdout patterns.  No test file imports another; the cases
and the assertions stay in the test files."""
import ctypes as C
import re

import numpy as np

import cloudsc_amd as ca
import fields_compare_cases as cc
import fields_convert_cases as fc
import spp_cases as sp
import tendbuf_cases as tb

NAMES = [k for _, k in ca.VALIDATED]   # the 20 outputs and plude
KLEV = 137
DIAG = ca.DIAGNOSTIC_FLUX_FIELDS
KEPT = ca.selected_outputs(ca.OUTPUTS_PROGNOSTIC)
ALL21 = ca.selected_outputs(ca.OUTPUTS_ALL)
KEPT_OTHER = ("plude", "pcovptot", "prainfrac_toprfz", "pfplsl", "pfplsn", "pfhpsl", "pfhpsn")
SENTINEL = 0xA7
CANARY = 0xC3
SURF = ca.OUTPUTS_SURFACE


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def columns(blocks, ngptot):
    return np.ascontiguousarray(ca.blocks_to_columns(blocks, ngptot))


def uses_aerosols(ds):
    return bool(ds.params.get("laericesed") or ds.params.get("laericeauto"))


def validation_table(out):
    """The CLI's validation table: the header row and everything after it."""
    lines = out.splitlines()
    start = [i for i, ln in enumerate(lines) if "Variable" in ln and "MaxRelErr" in ln][0]
    return lines[start:]


def full_fields(without=()):
    """A Fields with every member non-NULL but `without` (never dereferenced: the calls fail first)."""
    f = ca.Fields()
    for i, (n, _) in enumerate(ca.Fields._fields_):
        setattr(f, n, None if n in without else 0x1000 + 0x100 * i)
    return f


def configured(ds, case):
    import make_fixtures as mf
    s = ds.copy()
    s.params = dict(s.params)
    if case.startswith("nssopt"):
        s.params["nssopt"] = int(case[-1])
    elif case == "aerosol":
        s = mf.with_aerosols(ds)
    elif case == "aerosol_sed":
        s = mf.with_aerosols(ds)
        s.params["laericeauto"] = 0
    elif case == "aerosol_auto":
        s = mf.with_aerosols(ds)
        s.params["laericesed"] = 0
    elif case.startswith("ncldtop"):
        s.params["ncldtop"] = int(case[len("ncldtop"):])
    elif case.startswith("klev"):
        s = mf.sliced_levels(ds, ds.klev - int(case[4:]))
        s.params = dict(s.params)
        s.params["ncldtop"] = 2
    elif case in ("cold", "dry", "moist"):
        s = mf.shifted(ds, case)
    elif case.startswith("seed"):
        s = mf.perturbed(ds, int(case[4:]))
    else:
        raise ValueError(case)
    return s


# ---------------------------------------------------------------------------
# the host runs
# ---------------------------------------------------------------------------
_plain = {}


def plain_run(s, key, ngptot, nproma, precision):
    """cloudsc_cpu_run_precision on the dataset s (key: a name for it): {name: block-layout array}, once per
    case, read-only."""
    key = (key, ngptot, nproma, precision)
    if key not in _plain:
        st, _ = ca.cpu_run(s, ngptot, nproma, nthreads=4, precision=precision)
        for a in st.arrays.values():
            a.setflags(write=False)
        _plain[key] = st.arrays
    return _plain[key]


def run_selected(s, ngptot, nproma, precision, outputs, diag):
    """cloudsc_cpu_run_outputs on a fresh host state of s.  diag: "null" = the ten members NULL, "sentinel" =
    pointing at sentinel-filled arrays, "state" = the state's own arrays.  Returns the state's arrays with the
    ten members replaced by what the call was given (None for NULL)."""
    st = ca.make_host_state(s, ngptot, nproma, precision)
    # every output lane starts as sentinel bytes: padding lanes must keep them
    for n in ALL21:
        if n != "plude":
            bits(st.arrays[n])[...] = SENTINEL
    f = st.fields()
    given = dict(st.arrays)
    for n in DIAG:
        if diag == "null":
            setattr(f, n, None)
            given[n] = None
        elif diag == "sentinel":
            a = np.empty_like(st.arrays[n])
            bits(a)[...] = SENTINEL
            setattr(f, n, a.ctypes.data)
            given[n] = a
    ca.cpu_run_outputs(ca.Params.from_dict(s.params), f, precision, outputs, ngptot, nproma, s.klev, nthreads=3)
    return given


def check_kept(got, ref, ngptot, nproma, names=KEPT):
    bad = {}
    for k in names:
        if not np.array_equal(bits(columns(got[k], ngptot)), bits(columns(ref[k], ngptot))):
            bad[k] = "differs from cloudsc_cpu_run_precision"
        if ngptot % nproma and k != "plude":     # padding lanes of the last block keep the sentinel
            pad = got[k][-1][..., ngptot % nproma:]
            if not (bits(pad) == SENTINEL).all():
                bad[k] = "padding lanes written"
    assert bad == {}


def run_tendbuf_checked(ds, ngptot, nproma, precision, tend_planes, order, key="ds"):
    """cloudsc_cpu_run_tendbuf on the dataset (key: a name for it), checked against cloudsc_cpu_run_precision
    and for the sentinels; returns {name: block-layout array} of the 21 fields."""
    ref = plain_run(ds, key, ngptot, nproma, precision)
    st = ca.make_host_state(ds, ngptot, nproma, precision)
    nb, dt = ca.nblocks_of(ngptot, nproma), ca.storage_dtype(precision)
    lay = tb.layout(order, tend_planes)
    buf_tmp = tb.empty_buffer(nb, tend_planes, ds.klev, nproma, dt, tb.SENTINEL_TMP)
    buf_loc = tb.empty_buffer(nb, tend_planes, ds.klev, nproma, dt, tb.SENTINEL_LOC)
    for n in tb.TMP:
        tb.put(buf_tmp, lay[n], st.arrays[n], ngptot)
    tmp_before = buf_tmp.copy()
    f = st.fields()
    if order == "reference":
        ca.bind_tendbuf(f, precision, nproma, ds.klev, buf_tmp.ctypes.data, buf_loc.ctypes.data)
    else:
        tb.bind(f, lay, buf_tmp, buf_loc)
    ca.cpu_run_tendbuf(ca.Params.from_dict(ds.params), f, precision, ngptot, nproma, ds.klev, tend_planes,
                       nthreads=3)
    assert np.array_equal(tb.bits(buf_tmp), tb.bits(tmp_before))            # inputs are only read
    assert tb.is_sentinel(buf_loc, tb.untouched_mask(buf_loc, lay, tb.LOC, ngptot), tb.SENTINEL_LOC)
    got = {k: tb.take(buf_loc, lay[k], k) if k in tb.LOC else st.arrays[k] for k in NAMES}
    bad = {}
    for k in NAMES:
        if not np.array_equal(tb.bits(columns(got[k], ngptot)), tb.bits(columns(ref[k], ngptot))):
            bad[k] = "differs from cloudsc_cpu_run_precision"
    assert bad == {}
    return got


def host_set(s, ngptot, nproma, precision, tend_planes, order, outputs, loc):
    """The host state of one fused run: BUFFER_TMP filled, the separate tendency arrays and the diagnostic
    fluxes out of reach, tendency_loc_* NULL (loc "null") or bound to a canary-filled BUFFER_LOC ("canary");
    with SURFACE the four flux members are surface fields.  Returns (state, fields, buf_tmp, buf_loc)."""
    st = ca.make_host_state(s, ngptot, nproma, precision)
    nb, dt = ca.nblocks_of(ngptot, nproma), ca.storage_dtype(precision)
    lay = tb.layout(order, tend_planes)
    buf_tmp = tb.empty_buffer(nb, tend_planes, s.klev, nproma, dt, tb.SENTINEL_TMP)
    buf_loc = tb.empty_buffer(nb, tend_planes, s.klev, nproma, dt, CANARY)
    for n in tb.TMP:
        tb.put(buf_tmp, lay[n], st.arrays[n], ngptot)
    for n in tb.TMP + tb.LOC + tuple(DIAG):
        st.arrays[n].view(np.uint8)[...] = SENTINEL
    if outputs == SURF:
        for n in ca.SURFACE_FLUX_FIELDS:
            st.arrays[n] = np.full((nb, nproma), np.nan, dtype=dt)
    f = st.fields()
    tb.bind(f, lay, buf_tmp, buf_loc)
    for n in DIAG:
        setattr(f, n, None)
    if loc == "null":
        for n in tb.LOC:
            setattr(f, n, None)
    return st, f, buf_tmp, buf_loc


def oracle_step(oracle_mod, ngptot, nproma):
    """step(dataset) -> {name: [..][ngptot]} of the fp64 oracle."""
    def step(s):
        st, _ = oracle_mod.run_oracle(s, ngptot, nproma)
        return {k: columns(st.arrays[k], ngptot) for k in NAMES}
    return step


# ---------------------------------------------------------------------------
# the host sides of the tendency-buffer conversions and comparisons
# ---------------------------------------------------------------------------
CONV_KLEV = 3
CONV_NGPTOT = 150


class Side:
    """One side of a conversion on the host: every member in block layout of `nproma` columns, the
    tendency members in two packed buffers when tend_planes is non-zero."""

    def __init__(self, precision, nproma, tend_planes, order="reference", values=True, ngptot=CONV_NGPTOT):
        self.precision, self.nproma, self.tend_planes, self.ngptot = precision, nproma, tend_planes, ngptot
        self.nb = ca.nblocks_of(ngptot, nproma)
        self.arrays, self.f = {}, ca.Fields()
        for name in fc.MEMBERS:
            dt = fc.dtype_of(name, precision)
            cols = fc.encoded(name, fc.rows_of(name, CONV_KLEV), ngptot).astype(dt)
            a = fc.to_blocks(cols, nproma, dt, fc.POISON if values else bytes([tb.SENTINEL_LOC]))
            if not values:
                a.view(np.uint8)[...] = tb.SENTINEL_LOC
            self.arrays[name] = a
            setattr(self.f, name, a.ctypes.data)
        self.lay, self.bufs = None, None
        if tend_planes:
            dt = ca.storage_dtype(precision)
            self.lay = tb.layout(order, tend_planes)
            self.bufs = [tb.empty_buffer(self.nb, tend_planes, CONV_KLEV, nproma, dt, s)
                         for s in (tb.SENTINEL_TMP, tb.SENTINEL_LOC)]
            if values:
                for names, buf in ((tb.TMP, self.bufs[0]), (tb.LOC, self.bufs[1])):
                    for n in names:
                        tb.put(buf, self.lay[n], self.arrays[n], ngptot)
            tb.bind(self.f, self.lay, *self.bufs)

    def member(self, name):
        """The member as a block-layout array, wherever it lives."""
        if self.tend_planes and name in tb.TMP + tb.LOC:
            return tb.take(self.bufs[0] if name in tb.TMP else self.bufs[1], self.lay[name], name)
        return self.arrays[name]

    def snapshot(self):
        return [a.copy() for a in list(self.arrays.values()) + (self.bufs or [])]


def convert(src, dst):
    ca.cpu_convert_fields_tendbuf(src.f, dst.f, src.ngptot, CONV_KLEV, src.precision, src.nproma, src.tend_planes,
                                  dst.precision, dst.nproma, dst.tend_planes, nthreads=3)


def same_storage(got, want):
    return all(np.array_equal(tb.bits(g), tb.bits(w)) for g, w in zip(got, want))


# (src precision, NPROMA, planes, order) -> (dst precision, NPROMA, planes, order)
CONV_CASES = {
    "pack": ((ca.FP64, 64, 0, "reference"), (ca.FP64, 64, 8, "reference")),
    "unpack": ((ca.FP64, 64, 11, "permuted"), (ca.FP64, 64, 0, "reference")),
    "pack_reblock_24_64": ((ca.FP64, 24, 0, "reference"), (ca.FP64, 64, 11, "permuted")),
    "unpack_reblock_24_64": ((ca.FP32, 24, 8, "permuted"), (ca.FP32, 64, 0, "reference")),
    "pack_narrow_fp64_float": ((ca.FP64, 64, 0, "reference"), (ca.MIXED, 64, 8, "permuted")),
    "unpack_narrow_fp64_float": ((ca.FP64, 16, 11, "reference"), (ca.MIXED, 64, 0, "reference")),
    "repack_8_11": ((ca.FP64, 64, 8, "reference"), (ca.FP64, 24, 11, "permuted")),
}


class PackedSide:
    """A fields_convert_cases.HostSet whose tendency members may live in two packed buffers instead
    (tend_planes != 0): f points there; view() is the set as the comparison must see it, read back from
    the whole buffers."""

    def __init__(self, hs, tend_planes, order="permuted"):
        self.hs, self.tend_planes = hs, tend_planes
        self.arrays = hs.arrays
        self.f = hs.fields()
        self.lay, self.bufs = None, None
        if tend_planes:
            dt = ca.storage_dtype(hs.precision)
            nb = ca.nblocks_of(hs.ngptot, hs.nproma)
            self.lay = tb.layout(order, tend_planes)
            self.bufs = [tb.empty_buffer(nb, tend_planes, hs.klev, hs.nproma, dt, s)
                         for s in (tb.SENTINEL_TMP, tb.SENTINEL_LOC)]
            for names, buf in ((tb.TMP, self.bufs[0]), (tb.LOC, self.bufs[1])):
                for n in names:
                    if n in hs.names:
                        tb.put(buf, self.lay[n], hs.arrays[n], hs.ngptot)
                        hs.arrays[n].view(np.uint8)[...] = 0x3C      # the separate array is not the member now
            bound = ca.Fields()
            tb.bind(bound, self.lay, *self.bufs)
            for n in tb.TMP + tb.LOC:
                if n in hs.names:
                    setattr(self.f, n, getattr(bound, n))

    def buffer_of(self, name):
        return self.bufs[0 if name in tb.TMP else 1]

    def view(self):
        """An object restate() reads: names, ngptot, arrays in block layout."""
        class V:
            pass
        v = V()
        v.names, v.ngptot, v.nproma = self.hs.names, self.hs.ngptot, self.hs.nproma
        v.arrays = {}
        for n in self.hs.names:
            if self.tend_planes and n in tb.TMP + tb.LOC:
                a = tb.take(self.buffer_of(n), self.lay[n], n)
                v.arrays[n] = a.reshape(a.shape[0], -1, a.shape[-1])
            else:
                v.arrays[n] = self.hs.arrays[n]
        return v


def cpu_compare(a, b, nthreads=3):
    diffs = cc.new_diffs()
    ca.check(ca.gpu_lib().cloudsc_cpu_fields_compare_tendbuf(
        nthreads, a.hs.ngptot, a.hs.klev, a.hs.precision, a.hs.nproma, a.tend_planes, C.byref(a.f), b.hs.precision,
        b.hs.nproma, b.tend_planes, C.byref(b.f), diffs))
    return diffs


# ---------------------------------------------------------------------------
# the argument rules of cloudsc_gpu_run_spp (no launch: with and without a GPU)
# ---------------------------------------------------------------------------
def full_spp(**kw):
    s = ca.Spp()
    for i, n in enumerate(sp.SLOTS):
        setattr(s, n, kw.get(n, 0x900000 + 0x100 * i))
    return s


def gpu_run_spp_rules(lib):
    f = full_fields()
    ws = C.c_void_p(0x10)

    def run(prec=ca.FP64, variant=ca.VARIANT_KSEG, outputs=ca.OUTPUTS_PROGNOSTIC, ngptot=100, nproma=16, klev=KLEV,
            fields=f, spp=full_spp(), scratch=ws):
        return lib.cloudsc_gpu_run_spp(0, None, prec, variant, outputs, ngptot, nproma, klev,
                                       C.byref(fields) if fields is not None else None,
                                       C.byref(spp) if spp is not None else None, scratch)
    before = lib.cloudsc_last_hip_error()
    for outputs in (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC):
        assert run(outputs=outputs, spp=None) == ca.EINVAL
        assert run(outputs=outputs, spp=full_spp(**{n: None for n in sp.SLOTS})) == ca.EINVAL
        assert run(outputs=outputs, spp=full_spp(rclcrit=f.plsm)) == ca.EINVAL
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
        assert run(outputs=outputs, scratch=None) == ca.EINVAL
        assert run(outputs=outputs, fields=full_fields(without=("pt",))) == ca.EINVAL
    assert run(outputs=ca.OUTPUTS_SURFACE) == ca.EINVAL
    for outputs in (2, -1, 99):
        assert run(outputs=outputs) == ca.EINVAL
    assert run(outputs=ca.OUTPUTS_ALL, fields=full_fields(without=("pfsqlf",))) == ca.EINVAL
    assert lib.cloudsc_last_hip_error() == before


# ---------------------------------------------------------------------------
# the reference benchmark harness's patterns (tests/test_stdout_contract.py)
# ---------------------------------------------------------------------------
# JUBE's built-in pattern macros (JUBE documentation, "Predefined patterns")
JUBE = {
    "jube_pat_int": r"([+-]?\d+)",
    "jube_pat_nint": r"(?:[+-]?\d+)",
    "jube_pat_fp": r"([+-]?(?:\d*\.?\d+(?:[eE][-+]?\d+)?|\d+\.))",
    "jube_pat_nfp": r"(?:[+-]?(?:\d*\.?\d+(?:[eE][-+]?\d+)?|\d+\.))",
}


def jube(pat):
    """Expand $jube_pat_* macros (longest names first: nint before int)."""
    for k in sorted(JUBE, key=len, reverse=True):
        pat = pat.replace("$" + k, JUBE[k])
    return pat


# timing_pattern (include_patternset.yml:159-171)
TIMING = {
    "thr_time": r"(?:$jube_pat_nint\s+){6}:\s+$jube_pat_int\s+(?:$jube_pat_nint\s+){2}@\s+(?:rank#$jube_pat_nint:)?core#",
    "thr_mflops": r"(?:$jube_pat_nint\s+){6}:\s+$jube_pat_nint\s+$jube_pat_int\s+$jube_pat_nint\s+@\s+(?:rank#$jube_pat_nint:)?core#",
    "tot_time": r"(?:$jube_pat_nint\s*x\s*)?(?:$jube_pat_nint\s+){6}:\s+$jube_pat_int\s+(?:$jube_pat_nint\s+){2}(?::\s+)?TOTAL(?!\s@)",
    "tot_mflops": r"(?:$jube_pat_nint\s*x\s*)?(?:$jube_pat_nint\s+){6}:\s+$jube_pat_nint\s+$jube_pat_int\s+$jube_pat_nint\s+(?::\s+)?TOTAL(?!\s@)",
    "tot_numomp": r"(?:$jube_pat_nint\s*x\s*)?$jube_pat_int\s+(?:$jube_pat_nint\s+){5}:\s+(?:$jube_pat_nint\s+){3}(?::\s+)?TOTAL(?!\s@)",
    "tot_ngptot": r"(?:$jube_pat_nint\s*x\s*)?$jube_pat_nint\s+$jube_pat_int\s+(?:$jube_pat_nint\s+){4}:\s+(?:$jube_pat_nint\s+){3}(?::\s+)?TOTAL(?!\s@)",
    "tot_ngpblks": r"(?:$jube_pat_nint\s*x\s*)?(?:$jube_pat_nint\s+){3}$jube_pat_int\s+(?:$jube_pat_nint\s+){2}:\s+(?:$jube_pat_nint\s+){3}(?::\s+)?TOTAL(?!\s@)",
    "tot_nproma": r"(?:$jube_pat_nint\s*x\s*)?(?:$jube_pat_nint\s+){4}$jube_pat_int\s+$jube_pat_nint\s+:\s+(?:$jube_pat_nint\s+){3}(?::\s+)?TOTAL(?!\s@)",
}

FIELDS = ["PLUDE", "PCOVPTOT", "PRAINFRAC_TOPRFZ", "PFSQLF", "PFSQIF", "PFCQLNG", "PFCQNNG", "PFSQRF", "PFSQSF",
          "PFCQRNG", "PFCQSNG", "PFSQLTUR", "PFSQITUR", "PFPLSL", "PFPLSN", "PFHPSL", "PFHPSN", "tendency_loc%a",
          "tendency_loc%q", "tendency_loc%T", "tendency_loc%cld"]
COLUMNS = ["min", "max", "abs_max_err", "avg_abs_err", "max_rel_err"]


def result_patterns():
    """results_pattern (include_patternset.yml:3-134): for each field, five
    patterns that capture one of MinValue .. MaxRelErr-% on its row."""
    out = {}
    for f in FIELDS:
        for i, col in enumerate(COLUMNS):
            nums = [r"$jube_pat_fp" if j == i else r"$jube_pat_nfp" for j in range(5)]
            out[(f, col)] = re.escape(f) + r"\s+\dD\d\s+" + r"\s+".join(nums)
    return out


def check_timing(out, nthreads, ngptot, nproma, nblocks):
    """Apply the timing patterns; returns the captured per-thread times."""
    thr = [int(m.group(1)) for m in re.finditer(jube(TIMING["thr_time"]), out)]
    thr_mf = [int(m.group(1)) for m in re.finditer(jube(TIMING["thr_mflops"]), out)]
    assert len(thr) == nthreads and len(thr_mf) == nthreads, (thr, thr_mf)
    tot = {k: [int(m.group(1)) for m in re.finditer(jube(v), out)] for k, v in TIMING.items() if k.startswith("tot")}
    assert all(len(v) == 1 for v in tot.values()), tot
    assert tot["tot_ngptot"] == [ngptot] and tot["tot_nproma"] == [nproma] and tot["tot_ngpblks"] == [nblocks]
    assert tot["tot_time"][0] >= 0 and tot["tot_mflops"][0] >= 0
    return thr, tot


def check_results(out):
    """Apply the result patterns: every field's five values are captured, and
    the dwarf's tolerance holds (MaxRelErr-% <= 100 * 10 eps)."""
    got = {}
    for (f, col), pat in result_patterns().items():
        flags = re.IGNORECASE if f.startswith("tendency") else 0
        m = re.findall(jube(pat), out, flags)
        assert len(m) == 1, (f, col, m)
        got[(f, col)] = float(m[0])
    for f in FIELDS:
        assert got[(f, "max_rel_err")] <= 100 * 10 * 2.220446049250313e-16, f
    return got
