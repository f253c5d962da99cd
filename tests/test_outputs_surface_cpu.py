"""CLOUDSC_OUTPUTS_SURFACE without a GPU: the argument rules of the five entry points that take a selection for
the value 5 (and the value 4, the surface bit alone, which stays unknown), and the host step with SURFACE
against cloudsc_cpu_run_precision on the same host state (and the fp64 oracle) -- on raw bits: the seven
full-size outputs whole, the four surface fields pfplsl, pfplsn, pfhpsl, pfhpsn against row klev of the full
step's profiles.  Destinations start as sentinel bytes, so padding lanes, non-NULL diagnostic members and a
guard behind each surface array show any store that should not be there (a profile-sized store among them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import tendbuf_cases as tb

KLEV = 137
SURF = ca.OUTPUTS_SURFACE
DIAG = ca.DIAGNOSTIC_FLUX_FIELDS
SFLUX = ca.SURFACE_FLUX_FIELDS
KEPT = ca.selected_outputs(SURF)
FULL7 = tuple(n for n in KEPT if n not in SFLUX)
SENTINEL = 0xA7
GUARD = 64          # guard elements behind the last element of a surface array
SHAPES = [(300, 64), (100, 16), (70, 32), (1, 1), (300, 300)]


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def no_device(lib):
    """No HIP device in this process: a call whose arguments pass every rule then stops at CLOUDSC_ENODEV and
    can be made with made-up pointers.  (With a device it would launch: never made there.)"""
    n = C.c_int(0)
    return lib.cloudsc_gpu_device_count(C.byref(n)) != 0 or n.value == 0


def columns(blocks, ngptot):
    return np.ascontiguousarray(ca.blocks_to_columns(blocks, ngptot))


def test_the_selection_and_the_shape_helper():
    assert (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC, ca.OUTPUTS_SURFACE) == (0, 1, 5)
    assert SFLUX == ("pfplsl", "pfplsn", "pfhpsl", "pfhpsn")
    assert KEPT == ca.selected_outputs(ca.OUTPUTS_PROGNOSTIC) and len(KEPT) == 11 and len(FULL7) == 7
    for bad in (2, 4, -1, 99):
        with pytest.raises(ValueError):
            ca.selected_outputs(bad)
        with pytest.raises(ValueError):
            ca.selected_field_shape("pfplsl", KLEV, 64, bad)
    for n in SFLUX:
        assert ca.selected_field_shape(n, KLEV, 64, SURF) == (64,)
        for o in (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC):
            assert ca.selected_field_shape(n, KLEV, 64, o) == (KLEV + 1, 64)
    for n, kind in ca.ALL_FIELDS.items():
        if n not in SFLUX:
            assert ca.selected_field_shape(n, KLEV, 48, SURF) == ca.field_shape(kind, KLEV, 48), n
    assert ca.selected_field_shape("pfsqlf", KLEV, 64) == (KLEV + 1, 64)
    with pytest.raises(KeyError):
        ca.selected_field_shape("nope", KLEV, 64, SURF)


# ---------------------------------------------------------------------------
# argument rules (no call here can launch or run: each fails first)
# ---------------------------------------------------------------------------
def full_fields(without=()):
    f = ca.Fields()
    for i, (n, _) in enumerate(ca.Fields._fields_):
        setattr(f, n, None if n in without else 0x1000 + 0x100 * i)
    return f


@pytest.mark.parametrize("tend_planes", [0, 8], ids=["arrays", "tendbuf"])
def test_gpu_run_surface_rules_need_no_gpu(lib, tend_planes):
    f = full_fields(without=DIAG)           # NULL diagnostic members are allowed: every failure below is another rule's
    ws = C.c_void_p(0x10)

    def run(prec=ca.FP64, variant=ca.VARIANT_KSEG, outputs=SURF, ngptot=100, nproma=16, klev=KLEV, fields=f, scratch=ws,
            planes=tend_planes):
        fp = C.byref(fields) if fields is not None else None
        if tend_planes:
            return lib.cloudsc_gpu_run_tendbuf_outputs(0, None, prec, variant, outputs, ngptot, nproma, klev, planes, fp,
                                                       scratch)
        return lib.cloudsc_gpu_run_outputs(0, None, prec, variant, outputs, ngptot, nproma, klev, fp, scratch)
    for outputs in (4, 2, 3, 6, 7, 13, -1, 99):
        assert run(outputs=outputs) == ca.EINVAL, outputs
    for prec in (ca.FP64, ca.FP32, ca.MIXED):
        for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE, 77, ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM,
                        ca.VARIANT_KCACHE | ca.FP32_EXACT_LIBM):
            assert run(prec=prec, variant=variant) == ca.EINVAL, (prec, variant)
    assert run(prec=99) == ca.EINVAL
    assert run(ngptot=0) == ca.EINVAL
    assert run(klev=1) == ca.EINVAL
    assert run(fields=None) == ca.EINVAL
    assert run(scratch=None) == ca.EINVAL
    if tend_planes:
        assert run(planes=7) == ca.EINVAL and run(planes=65) == ca.EINVAL
    for missing in KEPT + ("pt", "ktype"):        # the four surface members are required like every kept output
        assert run(fields=full_fields(without=DIAG + (missing,))) == ca.EINVAL, missing
    # with every rule met the call gets as far as the device: anything but an argument error
    # (no device: CLOUDSC_ENODEV; the parent answers CLOUDSC_EINVAL to the value 5 itself)
    if no_device(lib):
        assert run() not in (0, ca.EINVAL)


@pytest.mark.parametrize("tend_planes", [0, 8], ids=["arrays", "tendbuf"])
def test_cpu_run_surface_rules(lib, ds, tend_planes):
    f = full_fields(without=DIAG)
    p = ca.Params.from_dict(ds.params)

    def run(prec=ca.FP64, outputs=SURF, ngptot=100, nproma=16, klev=KLEV, params=p, fields=f, planes=tend_planes):
        pp = C.byref(params) if params is not None else None
        fp = C.byref(fields) if fields is not None else None
        if tend_planes:
            return lib.cloudsc_cpu_run_tendbuf_outputs(1, prec, outputs, ngptot, nproma, klev, planes, pp, fp)
        return lib.cloudsc_cpu_run_outputs(1, prec, outputs, ngptot, nproma, klev, pp, fp)
    for outputs in (4, 2, 3, 6, 7, -1, 99):
        assert run(outputs=outputs) == ca.EINVAL, outputs
    assert run(prec=ca.FP32) == ca.EINVAL
    assert run(prec=99) == ca.EINVAL
    assert run(ngptot=0) == ca.EINVAL
    assert run(nproma=0) == ca.EINVAL
    assert run(klev=1) == ca.EINVAL
    assert run(params=None) == ca.EINVAL
    assert run(fields=None) == ca.EINVAL
    if tend_planes:
        assert run(planes=7) == ca.EINVAL and run(planes=65) == ca.EINVAL
    for missing in KEPT:
        assert run(fields=full_fields(without=DIAG + (missing,))) == ca.EINVAL, missing


def test_fields_alloc_surface_rules_need_no_gpu(lib):
    f, rep = ca.Fields(), ca.Placement()

    def alloc(flags=ca.PLACE_NONE, outputs=SURF, fields=f, prec=ca.FP64, ngptot=100, nproma=16):
        return lib.cloudsc_fields_alloc_outputs(0, prec, ngptot, nproma, KLEV, flags, outputs,
                                                C.byref(fields) if fields is not None else None, C.byref(rep))
    assert alloc(outputs=4) == ca.EINVAL
    assert alloc(flags=4) == ca.EINVAL
    assert alloc(fields=None) == ca.EINVAL
    for kw in (dict(prec=99), dict(ngptot=0), dict(nproma=0)):     # cloudsc_fields_alloc's own errors, its own code
        a = dict(prec=ca.FP64, ngptot=100, nproma=16)
        a.update(kw)
        want = lib.cloudsc_fields_alloc(0, a["prec"], a["ngptot"], a["nproma"], KLEV, ca.PLACE_NONE, C.byref(f),
                                        C.byref(rep))
        assert want != 0 and alloc(**kw) == want, kw
    if no_device(lib):
        assert alloc() not in (0, ca.EINVAL)       # the value 5 is known: the device's answer


def test_validate_compare_convert_surface_rules_need_no_gpu(lib):
    f = full_fields(without=DIAG)
    g = full_fields(without=DIAG)
    for i, (n, _) in enumerate(ca.Fields._fields_):
        if getattr(g, n):
            setattr(g, n, 0x100000 + 0x100 * i)
    diffs = (ca.FieldDiff * len(ca.ALL_FIELDS))()
    for outputs in (4, 2, -1, 99):
        assert lib.cloudsc_fields_compare_outputs(0, None, 100, KLEV, outputs, ca.FP64, 16, C.byref(f), ca.FP64, 16,
                                                  C.byref(g), diffs) == ca.EINVAL
        assert lib.cloudsc_fields_convert_outputs(0, None, 100, KLEV, outputs, ca.FP64, 16, C.byref(f), ca.FP64, 16,
                                                  C.byref(g)) == ca.EINVAL
    for outputs in (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC, SURF):
        assert lib.cloudsc_fields_compare_outputs(0, None, 100, KLEV, outputs, ca.FP64, 16, C.byref(f), ca.FP64, 16,
                                                  C.byref(g), None) == ca.EINVAL               # no diff[]
        assert lib.cloudsc_fields_compare_outputs(0, None, 0, KLEV, outputs, ca.FP64, 16, C.byref(f), ca.FP64, 16,
                                                  C.byref(g), diffs) == ca.EINVAL
        assert lib.cloudsc_fields_convert_outputs(0, None, 100, KLEV, outputs, 99, 16, C.byref(f), ca.FP64, 16,
                                                  C.byref(g)) == ca.EINVAL
        assert lib.cloudsc_fields_convert_outputs(0, None, 100, KLEV, outputs, ca.FP64, 16, C.byref(f), ca.FP64, 16,
                                                  C.byref(f)) == ca.EINVAL                     # the same arrays
        one = ca.fields_subset(f, ["pfplsl"])                                                 # NULL in one set only
        assert lib.cloudsc_fields_compare_outputs(0, None, 100, KLEV, outputs, ca.FP64, 16, C.byref(one), ca.FP64, 16,
                                                  C.byref(ca.Fields()), diffs) == ca.EINVAL
    keep = []
    ref = ca.Reference()
    stats = (ca.Stats * len(ca.VALIDATED))()
    for outputs in (4, 2, 99):
        assert lib.cloudsc_fields_validate_tendbuf(0, None, ca.FP64, 100, 16, KLEV, 0, outputs, 0, C.byref(f),
                                                   C.byref(ref), stats) == ca.EINVAL
    # SURFACE: a surface member without its reference profile (an empty reference) is an argument error
    ref.klon, ref.klev = 100, KLEV
    assert lib.cloudsc_fields_validate_tendbuf(0, None, ca.FP64, 100, 16, KLEV, 0, SURF, 0, C.byref(f), C.byref(ref),
                                               stats) == ca.EINVAL
    del keep


# ---------------------------------------------------------------------------
# the host step
# ---------------------------------------------------------------------------
_plain = {}


def plain_run(s, key, ngptot, nproma, precision):
    """cloudsc_cpu_run_precision on the dataset s: {name: block-layout array}, once per case, read-only."""
    key = (key, ngptot, nproma, precision)
    if key not in _plain:
        st, _ = ca.cpu_run(s, ngptot, nproma, nthreads=4, precision=precision)
        for a in st.arrays.values():
            a.setflags(write=False)
        _plain[key] = st.arrays
    return _plain[key]


def guarded_surface(nb, nproma, dtype):
    """A sentinel-filled [nb][nproma] array followed by GUARD sentinel elements in the same allocation."""
    raw = np.empty(nb * nproma + GUARD, dtype=dtype)
    bits(raw)[...] = SENTINEL
    return raw, raw[:nb * nproma].reshape(nb, nproma)


def run_surface(s, ngptot, nproma, precision, diag, tend_planes=0, order="reference"):
    """The host step with SURFACE on a fresh host state of s whose outputs start as sentinel bytes.  diag: the
    ten diagnostic members "null" or "sentinel".  tend_planes: the tendencies in two packed buffers.  Checks the
    guards, the diagnostic members and the buffers' untouched parts; returns {name: block-layout array} of
    the eleven kept outputs, the four surface members [nblocks][nproma]."""
    st = ca.make_host_state(s, ngptot, nproma, precision)
    nb, dt = ca.nblocks_of(ngptot, nproma), ca.storage_dtype(precision)
    for n in ca.selected_outputs(ca.OUTPUTS_ALL):
        if n != "plude":
            bits(st.arrays[n])[...] = SENTINEL
    f = st.fields()
    got = {n: st.arrays[n] for n in FULL7}
    raws = {}
    for n in SFLUX:
        raws[n], got[n] = guarded_surface(nb, nproma, dt)
        setattr(f, n, raws[n].ctypes.data)
    if diag == "null":
        for n in DIAG:
            setattr(f, n, None)
    p = ca.Params.from_dict(s.params)
    if tend_planes:
        lay = tb.layout(order, tend_planes)
        buf_tmp = tb.empty_buffer(nb, tend_planes, s.klev, nproma, dt, tb.SENTINEL_TMP)
        buf_loc = tb.empty_buffer(nb, tend_planes, s.klev, nproma, dt, tb.SENTINEL_LOC)
        for n in tb.TMP:
            tb.put(buf_tmp, lay[n], st.arrays[n], ngptot)
        tmp_before = buf_tmp.copy()
        for n in tb.TMP + tb.LOC:
            bits(st.arrays[n])[...] = SENTINEL                      # the separate arrays are not the run's
        tb.bind(f, lay, buf_tmp, buf_loc)
        ca.cpu_run_tendbuf_outputs(p, f, precision, SURF, ngptot, nproma, s.klev, tend_planes, nthreads=3)
        assert np.array_equal(tb.bits(buf_tmp), tb.bits(tmp_before))
        assert tb.is_sentinel(buf_loc, tb.untouched_mask(buf_loc, lay, tb.LOC, ngptot), tb.SENTINEL_LOC)
        for n in tb.TMP + tb.LOC:
            assert (bits(st.arrays[n]) == SENTINEL).all(), n
        for n in tb.LOC:
            got[n] = tb.take(buf_loc, lay[n], n)
    else:
        ca.cpu_run_outputs(p, f, precision, SURF, ngptot, nproma, s.klev, nthreads=3)
    for n in DIAG + SFLUX:                  # the state's own profile-sized arrays: every byte kept
        assert (bits(st.arrays[n]) == SENTINEL).all(), n
    for n in SFLUX:                         # nothing behind the last element of a surface array
        assert (bits(raws[n][nb * nproma:]) == SENTINEL).all(), n
    return got


def check_surface(got, ref, ngptot, nproma, klev, in_buffers=()):
    """got (run_surface) against the full step's arrays ref, on raw bits; padding lanes keep the sentinel."""
    bad = {}
    for k in FULL7:
        if not np.array_equal(bits(columns(got[k], ngptot)), bits(columns(ref[k], ngptot))):
            bad[k] = "differs from the full step"
    for k in SFLUX:
        want = ref[k][:, klev, :]                                   # row klev of [nblocks][klev+1][nproma]
        assert got[k].shape == want.shape
        if not np.array_equal(bits(columns(got[k], ngptot)), bits(columns(want, ngptot))):
            bad[k] = "differs from row klev of the full step's profile"
    if ngptot % nproma:
        for k in KEPT:
            if k == "plude" or k in in_buffers:
                continue
            if not (bits(got[k][-1][..., ngptot % nproma:]) == SENTINEL).all():
                bad[k] = "padding lanes written"
    assert bad == {}


@pytest.mark.parametrize("diag", ["null", "sentinel"])
@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED], ids=["fp64", "mixed"])
@pytest.mark.parametrize("ngptot,nproma", SHAPES)
def test_cpu_run_surface_bitwise(ds, oracle_mod, ngptot, nproma, precision, diag):
    ref = plain_run(ds, "ds", ngptot, nproma, precision)
    got = run_surface(ds, ngptot, nproma, precision, diag)
    check_surface(got, ref, ngptot, nproma, ds.klev)
    if precision == ca.FP64:
        ost, _ = oracle_mod.run_oracle(ds, ngptot, nproma)
        check_surface(got, ost.arrays, ngptot, nproma, ds.klev)
        # the surface precipitation of the dataset is not all zero: the comparison above saw real values
        assert np.count_nonzero(columns(got["pfplsl"], ngptot)) + np.count_nonzero(columns(got["pfplsn"], ngptot)) > 0 \
            or ngptot == 1


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED], ids=["fp64", "mixed"])
@pytest.mark.parametrize("ngptot,nproma", SHAPES)
def test_cpu_run_tendbuf_surface_bitwise(ds, ngptot, nproma, precision):
    ref = plain_run(ds, "ds", ngptot, nproma, precision)
    for tend_planes, order, diag in ((8, "reference", "null"), (11, "permuted", "sentinel")):
        got = run_surface(ds, ngptot, nproma, precision, diag, tend_planes, order)
        check_surface(got, ref, ngptot, nproma, ds.klev, in_buffers=tb.LOC)


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED], ids=["fp64", "mixed"])
def test_cpu_run_surface_with_aerosols(ds, oracle_mod, precision):
    import make_fixtures as mf
    s = mf.with_aerosols(ds)
    ref = plain_run(s, "aerosol", 300, 64, precision)
    check_surface(run_surface(s, 300, 64, precision, "null"), ref, 300, 64, s.klev)
    check_surface(run_surface(s, 300, 64, precision, "sentinel", 11, "permuted"), ref, 300, 64, s.klev,
                  in_buffers=tb.LOC)
    if precision == ca.FP64:
        ost, _ = oracle_mod.run_oracle(s, 300, 64)
        check_surface(run_surface(s, 300, 64, precision, "null"), ost.arrays, 300, 64, s.klev)


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED], ids=["fp64", "mixed"])
def test_cpu_run_surface_shallow_column(ds, precision):
    """KLEV 3 (the bottom three levels as a column of their own), the physics on at every level but the first."""
    import make_fixtures as mf
    s = mf.sliced_levels(ds, ds.klev - 3)
    s.params["ncldtop"] = 2
    assert s.klev == 3
    ref = plain_run(s, "shallow", 100, 16, precision)
    check_surface(run_surface(s, 100, 16, precision, "null"), ref, 100, 16, 3)
    check_surface(run_surface(s, 100, 16, precision, "sentinel", 8, "reference"), ref, 100, 16, 3, in_buffers=tb.LOC)


# ---------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------
def validation_table(out):
    lines = out.splitlines()
    start = [i for i, ln in enumerate(lines) if "Variable" in ln and "MaxRelErr" in ln][0]
    return lines[start:]


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_cli_outputs_surface_on_the_host(ds, precision):
    """--outputs surface --variant cpu: the eleven kept rows, the four flux rows with Dim 1 and the statistics of
    the reference profiles' last row; the other seven rows are those of the full host step."""
    exe = os.path.join(os.path.dirname(ca.__file__), "dwarf-cloudsc-amd")
    base = [exe, "2", "300", "64", "--variant", "cpu", "--precision", precision]
    full = subprocess.run(base, capture_output=True, text=True, timeout=120)
    surf = subprocess.run(base + ["--outputs", "surface"], capture_output=True, text=True, timeout=120)
    assert full.returncode == 0 and surf.returncode == 0, (full.stderr, surf.stderr)
    ft, st = validation_table(full.stdout), validation_table(surf.stdout)
    assert len(ft) == 23 and len(st) == 13 and st[0] == ft[0]
    name = lambda ln: ln.split()[0].lower()
    assert [name(ln) for ln in st[1:-1]] == [name(ln) for ln in ft[1:-1] if name(ln) not in DIAG]
    by_name = {name(ln): ln for ln in ft[1:-1]}
    for ln in st[1:-1]:
        if name(ln) in SFLUX:
            assert ln.split()[1].startswith("1D"), ln          # a surface field, as PRAINFRAC_TOPRFZ
        else:
            assert ln == by_name[name(ln)]
    # the row's MinValue / MaxValue are those of the surface row of the host step's profile
    st_full, _ = ca.cpu_run(ds, 300, 64, nthreads=2, precision=ca.FP64 if precision == "fp64" else ca.MIXED)
    for ln in st[1:-1]:
        if name(ln) in SFLUX:
            row = columns(st_full.arrays[name(ln)][:, ds.klev, :], 300).astype(np.float64)
            cols = ln.split()
            assert float(cols[2]) == pytest.approx(row.min(), rel=1e-12, abs=0)
            assert float(cols[3]) == pytest.approx(row.max(), rel=1e-12, abs=0)
    assert st[-1].split("(")[0] == ft[-1].split("(")[0]
    if precision == "fp64":
        assert "VALIDATION: PASSED" in st[-1]
