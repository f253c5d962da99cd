"""CLOUDSC_OUTPUTS_SURFACE on the device: cloudsc_gpu_run_outputs / cloudsc_gpu_run_tendbuf_outputs with the value 5
against cloudsc_gpu_run on a second set holding the same inputs, on raw bits -- the seven full-size outputs whole,
the four surface fields pfplsl, pfplsn, pfhpsl, pfhpsn against row klev of the full step's profiles -- on the host
(with the pattern bytes of padding lanes, of non-NULL diagnostic members and of a guard behind every surface
array) and on the device (cloudsc_fields_compare_outputs); fp64 also against the oracle.  Then
cloudsc_fields_alloc_outputs, cloudsc_fields_validate_tendbuf and cloudsc_fields_convert_outputs for the
selection."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca
import form_state_cases as fs
import tendbuf_cases as tb
from gpu_harness import ALL21, CASES, DIAG, DeviceProblem, PATTERN, PRECISIONS, VARIANTS
from gpu_harness import columns, host_inputs, oracle_columns, raw_bits as bits
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SURF = ca.OUTPUTS_SURFACE
SFLUX = ca.SURFACE_FLUX_FIELDS
KEPT = ca.selected_outputs(SURF)
FULL7 = tuple(n for n in KEPT if n not in SFLUX)
GUARD = 64


class SurfaceSets(DeviceProblem):
    """One problem on the device in three sets with the same inputs and pattern-filled outputs:
      "all"      cloudsc_fields_alloc, run with cloudsc_gpu_run: the reference;
      "null"     cloudsc_fields_alloc_outputs(SURFACE): the ten diagnostic members NULL, the four surface members
                 [nblocks][nproma];
      "guarded"  all 21 allocated (the ten must keep every byte), the four surface members replaced by arrays of
                 this test's own with GUARD pattern elements behind the last element.
    tend_planes: "null" and "guarded" keep their tendencies in two packed buffers each (the "all" set does not)."""

    def __init__(self, lib, hip, ds, ngptot, nproma, precision, tend_planes=0, place=False):
        super().__init__(lib, hip, ds, ngptot, nproma, precision)
        self.tend_planes = tend_planes
        self.host = host_inputs(ds, ngptot, nproma, precision, PATTERN)
        small = np.empty((self.nb, nproma), dtype=self.dt)
        bits(small)[...] = PATTERN
        surf_host = {n: (small if n in SFLUX else a) for n, a in self.host.items()}
        self.sets = {
            "all": self.device_fields(),
            "null": self.device_fields(place=place, outputs=SURF, tend_planes=tend_planes),
            "guarded": self.device_fields(tend_planes=tend_planes),
        }
        self.sets["all"].upload(self.host)
        self.upload(self.sets["null"], surf_host)
        self.upload(self.sets["guarded"], self.host)
        # the guarded set's surface members: [nb * nproma + GUARD] pattern elements each
        self.profile = {n: getattr(self.sets["guarded"].f, n) for n in SFLUX}
        self.guarded = {n: self.device_array(np.full(self.nb * nproma + GUARD, 0, dtype=self.dt), PATTERN) for n in SFLUX}
        for n in SFLUX:
            setattr(self.sets["guarded"].f, n, self.guarded[n])

    def upload(self, dset, host):
        """The host arrays into a set; a tend_planes set: its separate arrays, then tendency_tmp_* packed into
        BUFFER_TMP, and both buffers' other bytes a pattern first."""
        if not dset.tend_planes:
            dset.upload(host)
            return
        f = dset.f
        dset.f = dset.separate
        try:
            dset.upload(host)
        finally:
            dset.f = f
        for buf, pat in ((dset.buffer_tmp, tb.SENTINEL_TMP), (dset.buffer_loc, tb.SENTINEL_LOC)):
            assert self.hip.hipMemset(C.c_void_p(buf), pat, C.c_size_t(dset.tendbuf_nbytes())) == 0
        ca.convert_fields_tendbuf(ca.fields_subset(dset.separate, tb.TMP), ca.fields_subset(dset.f, tb.TMP), self.ngptot,
                                  self.ds.klev, self.precision, self.nproma, 0, self.precision, self.nproma,
                                  dset.tend_planes)
        self.hip.hipDeviceSynchronize()

    def run(self, which, variant, outputs, stream=None):
        """One step on a set (cloudsc_gpu_run for outputs None), followed by its check."""
        d = self.sets[which]
        self.checked_step(d.f, variant, outputs, d.tend_planes if outputs is not None else 0, stream)

    def surface(self, which, name):
        """A surface member of "null" / "guarded" as [nb][nproma] (raw storage type)."""
        if which == "guarded":
            return self.read(self.guarded[name], self.nb * self.nproma + GUARD)[:self.nb * self.nproma].reshape(
                self.nb, self.nproma)
        return self.sets[which].download_raw(name)

    def full(self, which, name):
        """A full-size output of a set in block layout (a tend_planes set: tendency_loc_* out of BUFFER_LOC)."""
        d = self.sets[which]
        if d.tend_planes and name in tb.LOC:
            buf = self.read(d.buffer_loc, self.nb * d.tend_planes * self.ds.klev * self.nproma).reshape(
                self.nb, d.tend_planes, self.ds.klev, self.nproma)
            return tb.take(buf, tb.layout("reference", d.tend_planes)[name], name), buf
        return d.download_raw(name), None

    def host_check(self, which, oracle=None):
        """Raw bits against the "all" set, whole arrays with their padding lanes; the pattern bytes."""
        wrong = []
        tail = self.ngptot % self.nproma
        d = self.sets[which]
        for k in FULL7:
            got, buf = self.full(which, k)
            ref = self.sets["all"].download_raw(k)
            if buf is None:
                if not np.array_equal(bits(got), bits(ref)):
                    wrong.append("%s: differs (padding included)" % k)
                if tail and not (bits(got[-1][..., tail:]) == PATTERN).all():
                    wrong.append("%s: a padding lane was written" % k)
            else:
                if not np.array_equal(bits(columns(got, self.ngptot)), bits(columns(ref, self.ngptot))):
                    wrong.append("%s: differs" % k)
                lay = tb.layout("reference", d.tend_planes)
                if not tb.is_sentinel(buf, tb.untouched_mask(buf, lay, tb.LOC, self.ngptot), tb.SENTINEL_LOC):
                    wrong.append("BUFFER_LOC: written outside the members' planes and columns")
            if oracle is not None and not np.array_equal(bits(columns(got, self.ngptot)), bits(oracle[k])):
                wrong.append("%s: differs from the oracle" % k)
        for k in SFLUX:
            got = self.surface(which, k)
            ref = self.sets["all"].download_raw(k)[:, self.ds.klev, :]
            if not np.array_equal(bits(columns(got, self.ngptot)), bits(columns(ref, self.ngptot))):
                wrong.append("%s: differs from row klev of the full step's profile" % k)
            if tail and not (bits(got[-1][tail:]) == PATTERN).all():
                wrong.append("%s: a padding lane was written" % k)
            if oracle is not None and not np.array_equal(bits(columns(got, self.ngptot)), bits(oracle[k][self.ds.klev])):
                wrong.append("%s: differs from the oracle's row klev" % k)
        if which == "guarded":
            for k in SFLUX:
                g = self.read(self.guarded[k], self.nb * self.nproma + GUARD)[self.nb * self.nproma:]
                if not (bits(g) == PATTERN).all():
                    wrong.append("%s: the guard behind the surface array was written" % k)
                prof = self.read(self.profile[k], self.nb * (self.ds.klev + 1) * self.nproma)
                if not (bits(prof) == PATTERN).all():
                    wrong.append("%s: the set's profile-sized array was written" % k)
            for k in DIAG:
                if not (bits(d.download_raw(k)) == PATTERN).all():
                    wrong.append("%s: written by a SURFACE run" % k)
        else:
            assert not any(getattr(d.f, n) for n in DIAG)
        if d.tend_planes:                       # the separate tendency_loc_* arrays are not the run's
            for k in tb.LOC:
                sep = self.read(getattr(d.separate, k), d.nbytes(k) // np.dtype(self.dt).itemsize)
                if not (bits(sep) == PATTERN).all():
                    wrong.append("%s: the separate array was written" % k)
        return wrong

    def device_mismatches(self, which, stream=None):
        """cloudsc_fields_compare_outputs(SURFACE) of the set's eleven kept members against the "all" set's seven
        and row klev of its four profiles (sliced on the host, uploaded as surface fields)."""
        d = self.sets[which]
        names7 = [n for n in FULL7 if not (d.tend_planes and n in tb.LOC)]     # (BUFFER_LOC: on the host, host_check)
        a = ca.fields_subset(d.f, names7)
        b = ca.fields_subset(self.sets["all"].f, names7)
        for n in SFLUX:
            setattr(a, n, getattr(d.f, n))
            row = np.ascontiguousarray(self.sets["all"].download_raw(n)[:, self.ds.klev, :])
            setattr(b, n, self.device_array(row))
        out = ca.compare_fields_outputs(a, b, self.ngptot, self.ds.klev, SURF, self.precision, self.nproma,
                                        self.precision, self.nproma, stream=stream)
        assert set(SFLUX) <= set(out) and all(out[n]["compared"] == self.ngptot for n in SFLUX)
        return {k: v["mismatches"] for k, v in out.items() if v["mismatches"]}

    def close(self):
        for n in SFLUX:                                  # the library's own arrays back before they are freed
            setattr(self.sets["guarded"].f, n, self.profile[n])
            if self.sets["guarded"].separate is not None:
                setattr(self.sets["guarded"].separate, n, self.profile[n])
        super().close()


def surface_parity(s, variant, oracle=None, stream=None, run_all=True):
    if run_all:
        s.run("all", variant, None, stream)
    for w in ("null", "guarded"):
        s.run(w, variant, SURF, stream)
        assert s.host_check(w, oracle) == [], w
        assert s.device_mismatches(w, stream) == {}, w
    # the step did something, and the surface row is not all zero
    assert not (bits(s.sets["all"].download_raw("pfsqlf")) == PATTERN).all()
    row = columns(s.surface("null", "pfplsl"), s.ngptot), columns(s.surface("null", "pfplsn"), s.ngptot)
    assert np.count_nonzero(row[0]) + np.count_nonzero(row[1]) > 0


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("ngptot,nproma,variant", CASES)
def test_run_outputs_surface_bitwise(lib, hip, ds, oracle_mod, ngptot, nproma, variant, precision):
    s = SurfaceSets(lib, hip, ds, ngptot, nproma, PRECISIONS[precision])
    try:
        if nproma == 32:
            ca.narrow_pack(1)
        geo = ca.launch_geometry(PRECISIONS[precision], VARIANTS[variant], ngptot, nproma, ds.klev)
        assert geo["pack"] == (64 // nproma if nproma <= 32 else 1)
        oracle = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma) if precision == "fp64" else None
        surface_parity(s, VARIANTS[variant], oracle)
    finally:
        s.close()


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("ngptot,nproma,variant", [c for c in CASES if c[:2] in ((300, 64), (100, 16), (200, 128))])
def test_run_tendbuf_outputs_surface_bitwise(lib, hip, ds, ngptot, nproma, variant, precision):
    s = SurfaceSets(lib, hip, ds, ngptot, nproma, PRECISIONS[precision], tend_planes=11)
    try:
        surface_parity(s, VARIANTS[variant])
    finally:
        s.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_surface_with_aerosols(lib, hip, ds, oracle_mod, variant, precision):
    import make_fixtures as mf
    sa = mf.with_aerosols(ds)
    for ngptot, nproma in ((300, 64), (100, 16)):
        s = SurfaceSets(lib, hip, sa, ngptot, nproma, PRECISIONS[precision])
        try:
            oracle = oracle_columns(oracle_mod, sa, "aerosol", ngptot, nproma) if precision == "fp64" else None
            surface_parity(s, VARIANTS[variant], oracle)
        finally:
            s.close()


def test_surface_on_a_non_default_stream(lib, hip, ds):
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0
    s = SurfaceSets(lib, hip, ds, 300, 64, ca.FP64)
    try:
        for variant in VARIANTS.values():
            surface_parity(s, variant, stream=st)
    finally:
        hip.hipStreamSynchronize(st)
        s.close()
        hip.hipStreamDestroy(st)


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_surface_row_comes_out_of_the_last_of_three_segments(lib, hip, ds, precision):
    """The 3-segment, 3-workgroup KSEG schedule: the carried precipitation fluxes cross two hand-offs."""
    for ngptot, nproma in ((300, 64), (100, 16)):
        s = SurfaceSets(lib, hip, ds, ngptot, nproma, PRECISIONS[precision])
        try:
            s.run("all", ca.VARIANT_KSEG, None)
            ca.kseg_schedule(3, 3)
            surface_parity(s, ca.VARIANT_KSEG, run_all=False)
        finally:
            ca.kseg_schedule(0, 0)
            s.close()


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_one_workspace_serves_all_three_selections(lib, hip, ds, precision):
    """ALL / SURFACE / PROGNOSTIC / ALL on one KSEG workspace, in that order."""
    s = SurfaceSets(lib, hip, ds, 200, 128, PRECISIONS[precision])
    try:
        v = ca.VARIANT_KSEG
        s.run("all", v, None)
        want = {k: s.sets["all"].download_raw(k).copy() for k in ALL21}
        for w in ("null", "guarded"):
            s.run(w, v, SURF)
            assert s.host_check(w) == [], w
        # PROGNOSTIC on the "all" set (its ten diagnostic members keep the bits the first run left)
        s.run("all", v, ca.OUTPUTS_PROGNOSTIC)
        s.run("null", v, SURF)
        assert s.host_check("null") == []
        s.sets["all"].upload(s.host)
        s.run("all", v, None)
        for k in ALL21:
            assert np.array_equal(bits(s.sets["all"].download_raw(k)), bits(want[k])), k
    finally:
        s.close()


@pytest.mark.parametrize("name", fs.STATES)
def test_surface_on_rain_and_land_states(lib, hip, ds, scenarios, oracle_mod, name):
    sd = fs.dataset(name, ds, scenarios)
    exp = fs.oracle_outputs(oracle_mod, name, sd)
    n = fs.NGPTOT
    for nproma, variant in ((64, ca.VARIANT_KSEG), (16, ca.VARIANT_KCACHE)):
        s = SurfaceSets(lib, hip, sd, n, nproma, ca.FP64)
        try:
            s.run("all", variant, None)
            for w in ("null", "guarded"):
                s.run(w, variant, SURF)
                assert s.host_check(w) == [], (w, nproma)
            for k in SFLUX:
                assert np.array_equal(bits(columns(s.surface("null", k), n)), bits(exp[k][sd.klev])), (k, nproma)
            if fs.rain_active(name):
                assert np.count_nonzero(columns(s.surface("null", "pfplsl"), n)) > 0
        finally:
            s.close()


@pytest.mark.parametrize("place", [False, True], ids=["no_search", "search"])
def test_fields_alloc_outputs_surface(lib, hip, ds, place):
    """The set cloudsc_fields_alloc_outputs(SURFACE) makes: ten NULL members, four small ones, the rest as ever --
    with and without the placement search, whose probe writes the small members as surface fields -- and a step
    on it."""
    s = SurfaceSets(lib, hip, ds, 300, 64, ca.FP64, place=place)
    try:
        d = s.sets["null"]
        assert not any(getattr(d.f, n) for n in DIAG)
        assert all(getattr(d.f, n) for n in KEPT)
        assert all(d.shape(n) == (64,) and d.nbytes(n) == s.nb * 64 * 8 for n in SFLUX)
        rep = d.report.to_dict()
        assert (rep["method"] == "rw-probe") == place or rep["method"] == "none"
        # the search's probe overwrote the outputs: the pattern again (the inputs are untouched by it)
        small = np.empty((s.nb, 64), dtype=s.dt)
        bits(small)[...] = PATTERN
        d.upload({n: (small if n in SFLUX else s.host[n]) for n in KEPT})
        surface_parity(s, ca.VARIANT_KSEG)
    finally:
        s.close()


def test_validate_tendbuf_surface_against_the_reference_row(lib, hip, ds):
    """cloudsc_fields_validate_tendbuf(outputs = SURFACE): the four surface fields against row klev of
    the reference profiles (the dataset's reference, the arrays of reference.h5), the ten diagnostic records the
    skipped record, the rest as for a full set."""
    d2 = ds
    n, nproma = 300, 64
    s = SurfaceSets(lib, hip, d2, n, nproma, ca.FP64)
    try:
        s.run("all", ca.VARIANT_KSEG, None)
        s.run("null", ca.VARIANT_KSEG, SURF)
        keep = []
        ref = ca.make_reference(d2, keep)
        full = ca.validate_fields_tendbuf(s.sets["all"].f, ref, ca.FP64, n, nproma, d2.klev, 0)
        ids = {k: i for i, (_, k) in enumerate(ca.VALIDATED)}
        for k in DIAG:
            ref.field[ids[k]] = None
        st = ca.validate_fields_tendbuf(s.sets["null"].f, ref, ca.FP64, n, nproma, d2.klev, 0, outputs=SURF)
        for k in DIAG:
            r = st[ids[k]]
            assert (r.minval, r.maxval, r.maxerr, r.errsum, r.refsum) == (np.finfo(np.float64).max,
                                                                          -np.finfo(np.float64).max, 0.0, 0.0, 0.0), k
        for k in FULL7:
            a, b = st[ids[k]], full[ids[k]]
            assert (a.minval, a.maxval, a.maxerr, a.errsum, a.refsum) == (b.minval, b.maxval, b.maxerr, b.errsum,
                                                                          b.refsum), k
        klon = d2.klon
        for k in SFLUX:
            got = columns(s.surface("null", k), n).astype(np.float64)
            row = np.asarray(d2.reference[k], dtype=np.float64).reshape(d2.klev + 1, klon)[d2.klev]
            want = row[np.arange(n) % klon]
            r = st[ids[k]]
            assert r.minval == got.min() and r.maxval == got.max(), k
            assert r.maxerr == np.abs(got - want).max(), k
            assert r.refsum == pytest.approx(np.abs(want).sum(), rel=1e-13), k
            assert r.errsum <= 1e-12 * max(r.refsum, 1e-300) or r.errsum < 1e-20, k      # the fp64 step validates
    finally:
        s.close()


def test_convert_outputs_surface_reblocks_the_surface_fields(lib, hip, ds):
    """cloudsc_fields_convert_outputs / DeviceFields.convert_to between two SURFACE sets: NPROMA 64 fp64 into
    NPROMA 48 mixed and fp64, the four surface members as 1-D fields."""
    n = 300
    s = SurfaceSets(lib, hip, ds, n, 64, ca.FP64)
    others = []
    try:
        s.run("null", ca.VARIANT_KSEG, SURF)
        src = s.sets["null"]
        for prec in (ca.FP64, ca.MIXED):
            dst = ca.DeviceFields(n, 48, ds.klev, prec, place=False, outputs=SURF)
            others.append(dst)
            src.convert_to(dst, names=KEPT)
            hip.hipDeviceSynchronize()
            for k in KEPT:
                a = columns(src.download_raw(k), n)
                b = columns(dst.download_raw(k), n)
                assert b.shape == a.shape and np.array_equal(b, a.astype(ca.storage_dtype(prec))), (k, prec)
            assert src.compare(dst, names=KEPT)["pfplsl"]["compared"] == n
            if prec == ca.FP64:
                assert all(v["mismatches"] == 0 for v in src.compare(dst, names=KEPT).values())
        full = ca.DeviceFields(n, 48, ds.klev, ca.FP64, place=False)
        others.append(full)
        with pytest.raises(ValueError):
            src.convert_to(full, names=KEPT)              # profiles on one side, surface fields on the other
        src.convert_to(full, names=FULL7)
    finally:
        for d in others:
            d.close()
        s.close()
