"""TEST INFRASTRUCTURE ONLY -- the device-side plumbing of the GPU tests, once: the `lib`, `hip` and
`restore_knobs` fixtures (a GPU test file takes them with `from gpu_harness import lib, hip, restore_knobs`),
the bit views, pattern-filled host inputs, the cached oracle columns, the KSEG workspace, and DeviceProblem, the
base of the tests' device-problem classes (field sets, parameters, workspace, own buffers, one checked step,
the comparisons, close).  The cases and the assertions stay in the test files."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca
import form_state_cases as fs
import mixed_expected as mx
import tendbuf_cases as tb
from host_harness import columns, uses_aerosols, validation_table  # noqa: F401  (one definition for both sides)

NAMES = [k for _, k in ca.VALIDATED]           # the 20 outputs and plude
DIAG = ca.DIAGNOSTIC_FLUX_FIELDS
KEPT = ca.selected_outputs(ca.OUTPUTS_PROGNOSTIC)
ALL21 = ca.selected_outputs(ca.OUTPUTS_ALL)
PRECISIONS = {"fp64": ca.FP64, "fp32": ca.FP32, "mixed": ca.MIXED}
VARIANTS = {"kcache": ca.VARIANT_KCACHE, "kseg": ca.VARIANT_KSEG}
# partial last block | two sub-blocks per block under KSEG | packed by default | packed on request | one wide block
SHAPES = [(300, 64), (200, 128), (100, 16), (70, 32), (300, 300)]
CASES = [(n, p, v) for (n, p) in SHAPES for v in VARIANTS if not (p > 256 and v == "kcache")]


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = ca.gpu_lib()
    assert ca.device_count() > 0
    return lib


def hip_library():
    """The HIP runtime of cloudsc_amd._hip() with the argtypes of every call the tests make."""
    h = ca._hip()
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    return h


@pytest.fixture(scope="module")
def hip():
    return hip_library()


@pytest.fixture(autouse=True)
def restore_knobs():
    """The process-wide knobs a test may have set, back at their defaults."""
    yield
    ca.narrow_pack(-1)
    ca.kseg_schedule(0, 0)
    ca.compare_grid(0)


# ---------------------------------------------------------------------------
# bits, columns, host inputs, the oracle
# ---------------------------------------------------------------------------
def raw_bits(a):
    """The bytes of an array's own storage."""
    return np.ascontiguousarray(a).view(np.uint8)


def widened_bits(a):
    """Raw bits of a field as downloaded (float64 holding the storage type's values: widening is injective)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def differing(got, ref, names, bits=raw_bits):
    """The members of `names` whose arrays in the two dicts are not the same bits."""
    return [k for k in names if not np.array_equal(bits(got[k]), bits(ref[k]))]


def host_inputs(ds, ngptot, nproma, precision, pattern, plude_padding=True, extra_blocks=0):
    """Block-layout host arrays of make_host_state with every byte of every pure output set to `pattern`,
    plude's lanes past the last column too (plude_padding), and `extra_blocks` whole pattern blocks behind
    every array."""
    st = ca.make_host_state(ds, ngptot, nproma, precision)
    nb = ca.nblocks_of(ngptot, nproma)
    out = {}
    for name, a in st.arrays.items():
        a = np.ascontiguousarray(a).copy()
        if name in ca.OUTPUT_FIELDS:
            raw_bits(a)[...] = pattern
        if name == "plude" and plude_padding:
            a[nb - 1, ..., ngptot - (nb - 1) * nproma:].view(np.uint8)[...] = pattern
        if extra_blocks:
            a = np.concatenate([a, np.repeat(a[:1], extra_blocks, axis=0)], axis=0)
            raw_bits(a[nb:])[...] = pattern
        out[name] = a
    return out


_oracle = {}


def oracle_columns(oracle_mod, ds, key, ngptot, nproma, precision=ca.FP64):
    """{field: [..][ngptot]} of the restatement's 21 outputs, once per (dataset key, shape, precision),
    read-only."""
    k = (key, ngptot, nproma, precision)
    if k not in _oracle:
        st, _ = oracle_mod.run_oracle(ds, ngptot, nproma, precision)
        _oracle[k] = {n: columns(st.arrays[n], ngptot) for n in ALL21}
        for a in _oracle[k].values():
            a.setflags(write=False)
    return _oracle[k]


# ---------------------------------------------------------------------------
# the KSEG workspace, one checked step
# ---------------------------------------------------------------------------
def kseg_workspace(lib, hip, precision, variant, ngptot, nproma, klev):
    """The workspace cloudsc_gpu_scratch_bytes asks for (NULL where the variant needs none), its first 256
    bytes zeroed as the first launch requires; the caller frees it."""
    ws = C.c_void_p()
    nbytes = lib.cloudsc_gpu_scratch_bytes(precision, variant & 0xff, ngptot, nproma, klev)
    assert nbytes >= 0
    if nbytes > 0:
        assert hip.hipMalloc(C.byref(ws), C.c_size_t(nbytes)) == 0
        assert hip.hipMemset(ws, 0, C.c_size_t(256)) == 0
    return ws


def init_params(lib, params):
    """The parameter set (a dict) as the device's default set."""
    p = ca.Params.from_dict(params)
    ca.check(lib.cloudsc_gpu_init(0, C.byref(p)))


def run_on(lib, hip, ds, df, variant):
    """cloudsc_gpu_run + cloudsc_gpu_check on a DeviceFields with the dataset's parameters."""
    init_params(lib, ds.params)
    ws = kseg_workspace(lib, hip, df.precision, variant, df.ngptot, df.nproma, df.klev)
    try:
        ca.check(lib.cloudsc_gpu_run(0, None, df.precision, variant, df.ngptot, df.nproma, df.klev, C.byref(df.f), ws))
        assert lib.cloudsc_gpu_check(0, None, variant, ws) == 0
    finally:
        if ws.value:
            hip.hipFree(ws)


class DeviceProblem:
    """One problem on the device: shape, precision, the dataset's parameters as the device's default set, the
    DeviceFields sets a subclass makes with device_fields(), device buffers of the test's own, the KSEG
    workspace, one step followed by its check, the device comparison; close() frees all of it."""

    def __init__(self, lib, hip, ds, ngptot, nproma, precision):
        self.lib, self.hip, self.ds = lib, hip, ds
        self.ngptot, self.nproma, self.precision, self.klev = ngptot, nproma, precision, ds.klev
        self.nb, self.dt = ca.nblocks_of(ngptot, nproma), ca.storage_dtype(precision)
        self.aer = uses_aerosols(ds)
        self.ws = C.c_void_p()
        self.own, self.field_sets = [], []
        self.init_params(ds.params)

    def init_params(self, params):
        init_params(self.lib, params)

    def device_fields(self, ngptot=None, place=False, **kw):
        """A DeviceFields of this problem's blocking and precision that close() closes."""
        d = ca.DeviceFields(ngptot or self.ngptot, self.nproma, self.klev, self.precision, place=place,
                            aerosols=self.aer, **kw)
        self.field_sets.append(d)
        return d

    def device_array(self, a, pattern=None):
        """A device copy of a host array (every byte `pattern`, if given) that close() frees: its address."""
        a = np.ascontiguousarray(a)
        if pattern is not None:
            raw_bits(a)[...] = pattern
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        self.own.append(p.value)
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value

    def read(self, ptr, like):
        """Device memory at `ptr` as a host array like `like` (a count: that many storage-type elements)."""
        out = np.empty(like, dtype=self.dt) if isinstance(like, int) else np.empty_like(like)
        self.hip.hipDeviceSynchronize()
        assert self.hip.hipMemcpy(out.ctypes.data, C.c_void_p(getattr(ptr, "value", ptr)), out.nbytes, 2) == 0
        return out

    def scratch(self, variant):
        if variant & 0xff == ca.VARIANT_KSEG and not self.ws.value:
            self.ws = kseg_workspace(self.lib, self.hip, self.precision, variant, self.ngptot, self.nproma, self.klev)
            assert self.ws.value
        return self.ws

    def checked_step(self, f, variant, outputs=None, tend_planes=0, stream=None, spp=None, cml=None):
        """One step on the Fields f through the entry its form has (outputs None: cloudsc_gpu_run /
        cloudsc_gpu_run_tendbuf), followed by cloudsc_gpu_check on the same stream and workspace."""
        ws, prec, shape = self.scratch(variant), self.precision, (self.ngptot, self.nproma, self.klev)
        if cml is not None:
            ca.gpu_run_tendbuf_cml(f, cml, prec, variant, outputs, *shape, tend_planes, scratch=ws, stream=stream)
        elif spp is not None:
            ca.gpu_run_spp(f, spp, prec, variant, outputs, *shape, scratch=ws, stream=stream)
        elif tend_planes and outputs is None:
            ca.gpu_run_tendbuf(f, prec, variant, *shape, tend_planes, scratch=ws, stream=stream)
        elif tend_planes:
            ca.gpu_run_tendbuf_outputs(f, prec, variant, outputs, *shape, tend_planes, scratch=ws, stream=stream)
        elif outputs is None:
            ca.check(self.lib.cloudsc_gpu_run(0, stream, prec, variant, *shape, C.byref(f), ws))
        else:
            ca.gpu_run_outputs(f, prec, variant, outputs, *shape, scratch=ws, stream=stream)
        assert self.lib.cloudsc_gpu_check(0, stream, variant & 0xff, ws) == 0

    def mismatches(self, a, b, names, stream=None, a_tend_planes=0):
        """cloudsc_fields_compare of `names` of the Fields a against b's (a_tend_planes: a's tendency members
        read in place from its packed buffers): {member: mismatches} where not 0."""
        a, b = ca.fields_subset(a, names), ca.fields_subset(b, names)
        shape = (self.ngptot, self.klev, self.precision, self.nproma)
        if a_tend_planes:
            d = ca.compare_fields_tendbuf(a, b, *shape, a_tend_planes, self.precision, self.nproma, 0, stream=stream)
        else:
            d = ca.compare_fields(a, b, *shape, self.precision, self.nproma, stream=stream)
        assert sorted(d) == sorted(names)
        assert all(v["compared"] > 0 for v in d.values())
        return {k: v["mismatches"] for k, v in d.items() if v["mismatches"]}

    def close(self):
        if self.ws.value:
            self.hip.hipFree(self.ws)
            self.ws = C.c_void_p()
        for s in self.field_sets:
            s.close()
        for p in self.own:
            self.hip.hipFree(C.c_void_p(p))
        self.own, self.field_sets = [], []


class DeviceSide:
    """A host_harness.Side or PackedSide mirrored on the device: plain hipMalloc copies of every array and buffer, the Fields
    pointing at the same places in them."""

    def __init__(self, hip, side):
        self.hip, self.side, self.f = hip, side, ca.Fields()
        self.host = list(side.arrays.values()) + (side.bufs or [])
        self.dev = []
        for a in self.host:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
            assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
            self.dev.append(p.value)
        for name, _ in ca.Fields._fields_:
            hp = getattr(side.f, name)
            if hp:
                setattr(self.f, name, self.translate(hp))

    def translate(self, host_ptr):
        for a, d in zip(self.host, self.dev):
            if a.ctypes.data <= host_ptr < a.ctypes.data + a.nbytes:
                return d + (host_ptr - a.ctypes.data)
        raise AssertionError("pointer outside every array")

    def snapshot(self):
        self.hip.hipDeviceSynchronize()
        out = []
        for a, d in zip(self.host, self.dev):
            b = np.empty_like(a)
            assert self.hip.hipMemcpy(b.ctypes.data, d, b.nbytes, 2) == 0
            out.append(b)
        return out

    def close(self):
        for d in self.dev:
            self.hip.hipFree(d)


# ---------------------------------------------------------------------------
# the device problems more than one test file runs
# ---------------------------------------------------------------------------
PATTERN = 0xC3              # the outputs of Pair and Sets before a step
RUN_PATTERN = 0xA5          # the outputs, padding lanes and extra blocks of Run before a step


class Pair(DeviceProblem):
    """One problem twice on the device: `plain` with separate tendency arrays, `packed` with the two
    tendency buffers of DeviceFields(tend_planes=...)."""

    def __init__(self, lib, hip, ds, ngptot, nproma, precision, tend_planes, order):
        super().__init__(lib, hip, ds, ngptot, nproma, precision)
        self.tend_planes = tend_planes
        self.host = host_inputs(ds, ngptot, nproma, precision, PATTERN)
        self.lay = tb.layout(order, tend_planes)
        self.plain = self.device_fields()
        self.packed = self.device_fields(tend_planes=tend_planes)
        self.buf_tmp = tb.empty_buffer(self.nb, tend_planes, ds.klev, nproma, self.dt, tb.SENTINEL_TMP)
        self.buf_loc = tb.empty_buffer(self.nb, tend_planes, ds.klev, nproma, self.dt, tb.SENTINEL_LOC)
        for n in tb.TMP:
            tb.put(self.buf_tmp, self.lay[n], self.host[n], ngptot)
        assert self.buf_tmp.nbytes == self.packed.tendbuf_nbytes()
        if order != "reference":       # the constructor bound the reference's planes
            plane = ds.klev * nproma * self.buf_tmp.itemsize
            for names, base in ((tb.TMP, self.packed.buffer_tmp), (tb.LOC, self.packed.buffer_loc)):
                for n in names:
                    setattr(self.packed.f, n, base + self.lay[n] * plane)

    def fill(self, which=("plain", "packed")):
        if "plain" in which:
            self.plain.upload(self.host)
        if "packed" in which:
            self.packed.upload({k: v for k, v in self.host.items() if not k.startswith("tendency_")})
            assert self.hip.hipMemcpy(self.packed.buffer_tmp, self.buf_tmp.ctypes.data, self.buf_tmp.nbytes, 1) == 0
            assert self.hip.hipMemcpy(self.packed.buffer_loc, self.buf_loc.ctypes.data, self.buf_loc.nbytes, 1) == 0

    def run_both(self, variant, stream=None, which=("plain", "packed")):
        """cloudsc_gpu_run on `plain`, cloudsc_gpu_run_tendbuf on `packed` (each followed by its check)."""
        if "plain" in which:
            self.checked_step(self.plain.f, variant, stream=stream)
        if "packed" in which:
            self.checked_step(self.packed.f, variant, tend_planes=self.tend_planes, stream=stream)

    def device_mismatches(self, stream=None):
        """Unpack BUFFER_LOC into the packed set's separate arrays, then cloudsc_fields_compare of its 21
        outputs against the plain set's: {member: mismatches} where not 0."""
        loc_src = ca.fields_subset(self.packed.f, tb.LOC)
        loc_dst = ca.fields_subset(self.packed.separate, tb.LOC)
        ca.convert_fields_tendbuf(loc_src, loc_dst, self.ngptot, self.ds.klev, self.precision, self.nproma,
                                  self.tend_planes, self.precision, self.nproma, 0, stream=stream)
        return self.mismatches(self.packed.separate, self.plain.f, NAMES, stream)

    def buffers(self):
        """BUFFER_TMP and BUFFER_LOC of the packed set as they are now."""
        return self.read(self.packed.buffer_tmp, self.buf_tmp), self.read(self.packed.buffer_loc, self.buf_loc)

    def host_check(self, names=NAMES):
        """The same on the host, and the sentinels: returns the list of what is wrong."""
        tmp, loc = self.buffers()
        wrong = []
        if not np.array_equal(tb.bits(tmp), tb.bits(self.buf_tmp)):
            wrong.append("BUFFER_TMP changed")
        if not tb.is_sentinel(loc, tb.untouched_mask(loc, self.lay, tb.LOC, self.ngptot), tb.SENTINEL_LOC):
            wrong.append("BUFFER_LOC: an unbound plane or a padding lane was written")
        for k in names:
            ref = self.plain.download_raw(k)
            if k in tb.LOC:
                got = tb.take(loc, self.lay[k], k)
            else:
                got = self.packed.download_raw(k)
                if not np.array_equal(tb.bits(got), tb.bits(ref)):    # whole arrays: padding lanes included
                    wrong.append("%s: differs (padding included)" % k)
            if not np.array_equal(tb.bits(columns(got, self.ngptot)), tb.bits(columns(ref, self.ngptot))):
                wrong.append("%s: differs" % k)
        return wrong


def without_diag(f):
    g = ca.Fields()
    C.memmove(C.byref(g), C.byref(f), C.sizeof(ca.Fields))
    for n in DIAG:
        setattr(g, n, None)
    return g


class ProgPair(Pair):
    """Pair whose packed set runs cloudsc_gpu_run_tendbuf_outputs."""

    def run_form(self, variant, outputs=ca.OUTPUTS_PROGNOSTIC, diag="null", stream=None):
        f = without_diag(self.packed.f) if diag == "null" else self.packed.f
        self.checked_step(f, variant, outputs, self.tend_planes, stream)

    def device_mismatches_inplace(self, names=KEPT, stream=None):
        """cloudsc_fields_compare_tendbuf of the packed set, BUFFER_LOC read in place, against the plain set:
        {member: mismatches} where not 0."""
        return self.mismatches(self.packed.f, self.plain.f, names, stream, a_tend_planes=self.tend_planes)

    def host_check_form(self, outputs=ca.OUTPUTS_PROGNOSTIC):
        """Pair.host_check of the selection's outputs, and the ten diagnostic members' pattern."""
        prog = outputs == ca.OUTPUTS_PROGNOSTIC
        wrong = self.host_check(KEPT if prog else NAMES)
        if prog:
            for k in DIAG:
                if not (raw_bits(self.packed.download_raw(k)) == PATTERN).all():
                    wrong.append("%s: a diagnostic member was written" % k)
        return wrong

    def kept_columns(self):
        loc = self.buffers()[1]
        return {k: columns(tb.take(loc, self.lay[k], k) if k in tb.LOC else self.packed.download_raw(k),
                           self.ngptot) for k in KEPT}


class Sets(DeviceProblem):
    """One problem on the device in several sets with the same inputs and pattern-filled outputs: "all"
    (cloudsc_fields_alloc), "null" (cloudsc_fields_alloc_outputs(PROGNOSTIC): the ten members NULL) and "kept"
    (all 21 allocated, run with PROGNOSTIC: the ten must keep the pattern)."""

    def __init__(self, lib, hip, ds, ngptot, nproma, precision, which=("all", "null", "kept")):
        super().__init__(lib, hip, ds, ngptot, nproma, precision)
        self.host = host_inputs(ds, ngptot, nproma, precision, PATTERN)
        self.sets = {}
        for w in which:
            self.sets[w] = self.device_fields(outputs=ca.OUTPUTS_PROGNOSTIC if w == "null" else ca.OUTPUTS_ALL)
            self.sets[w].upload(self.host)

    def run(self, which, variant, outputs, stream=None):
        """One step on a set (cloudsc_gpu_run for outputs None), followed by its check."""
        self.checked_step(self.sets[which].f, variant, outputs, stream=stream)

    def device_mismatches(self, which, names=KEPT, against="all", stream=None):
        """cloudsc_fields_compare of `names` of a set against the "all" set's: {member: mismatches} where not 0."""
        a = ca.fields_subset(self.sets[which].f, names)
        b = ca.fields_subset(self.sets[against].f, names)
        if names is KEPT:
            assert not any(getattr(a, n) or getattr(b, n) for n in DIAG)    # NULL in both operands
        return self.mismatches(a, b, names, stream)

    def host_check(self, which, names=KEPT, against="all", oracle=None):
        """The same on the host, whole arrays (padding lanes included), and the pattern bytes: padding lanes
        of every output, and every byte of a diagnostic member that was not to be written."""
        self.hip.hipDeviceSynchronize()
        wrong = []
        tail = self.ngptot % self.nproma
        for k in names:
            got, ref = self.sets[which].download_raw(k), self.sets[against].download_raw(k)
            if not np.array_equal(raw_bits(got), raw_bits(ref)):
                wrong.append("%s: differs (padding included)" % k)
            if tail and not (raw_bits(got[-1][..., tail:]) == PATTERN).all():
                wrong.append("%s: a padding lane was written" % k)
            if oracle is not None and not np.array_equal(raw_bits(columns(got, self.ngptot)), raw_bits(oracle[k])):
                wrong.append("%s: differs from the oracle" % k)
        if names is KEPT:
            for k in DIAG:
                if getattr(self.sets[which].f, k) and not (raw_bits(self.sets[which].download_raw(k)) == PATTERN).all():
                    wrong.append("%s: written by a PROGNOSTIC run" % k)
        return wrong


def prognostic_parity(s, variant, oracle=None, stream=None, run_all=True):
    """cloudsc_gpu_run on "all" (run_all False: the caller has run it), PROGNOSTIC on "null" and "kept"; the
    eleven kept members on the device and on the host."""
    if run_all:
        s.run("all", variant, None, stream)
    for w in ("null", "kept"):
        s.run(w, variant, ca.OUTPUTS_PROGNOSTIC, stream)
        assert not any(getattr(s.sets["null"].f, n) for n in DIAG)
        assert all(getattr(s.sets["kept"].f, n) for n in DIAG)
        assert s.device_mismatches(w, stream=stream) == {}, w
        assert s.host_check(w, oracle=oracle) == [], w
    # the step did something: the reference run wrote the diagnostic fluxes and the kept outputs
    assert not (raw_bits(s.sets["all"].download_raw("pfsqlf")) == PATTERN).all()
    assert not (raw_bits(s.sets["null"].download_raw("pfplsn")) == PATTERN).all()


def pattern_like(a):
    p = np.empty_like(a)
    p.view(np.uint8)[...] = RUN_PATTERN
    return p


class Run(DeviceProblem):
    """cloudsc_gpu_run on caller-owned buffers (DeviceFields) that are
    `extra_blocks` NPROMA blocks longer than the run needs.  Before every launch
    the inputs are uploaded again and every output buffer, plude's padding lanes
    and the extra blocks are filled with a byte pattern."""

    def __init__(self, lib, ds, ngptot, nproma, precision=ca.FP64, extra_blocks=0):
        super().__init__(lib, hip_library(), ds, ngptot, nproma, precision)
        self.df = self.device_fields((self.nb + extra_blocks) * nproma)
        self.host = host_inputs(ds, ngptot, nproma, precision, RUN_PATTERN, extra_blocks=extra_blocks)

    def launch(self, variant, pack, schedule=(0, 0)):
        """One step; returns {field: block-layout array of the WHOLE buffer}."""
        self.df.upload(self.host)
        ca.narrow_pack(pack)
        ca.kseg_schedule(*schedule)
        self.checked_step(self.df.f, variant)
        return {k: self.df.download(k) for k in NAMES}

    def columns(self, blocks):
        return {k: ca.blocks_to_columns(a[:self.nb], self.ngptot) for k, a in blocks.items()}


# ---------------------------------------------------------------------------
# the kernel forms on the states of tests/form_state_cases.py
# ---------------------------------------------------------------------------
def pack_of(s, precision, variant, nproma):
    return ca.launch_geometry(precision, variant, fs.NGPTOT, nproma, s.klev, laer=uses_aerosols(s))["pack"]


def plain_is_pinned(out, oracle_mod, name, s, precision):
    """The plain unpacked run ({field: [..][N]}) against the oracle (fp64) / the contract (mixed)."""
    if precision == ca.FP64:
        assert differing(out, fs.oracle_outputs(oracle_mod, name, s), fs.NAMES, widened_bits) == []
    elif precision == ca.MIXED:
        exp = mx.expected(oracle_mod, s, fs.NGPTOT, fs.ORACLE_NPROMA, key="forms:" + name)
        assert mx.mismatches(out, exp) == {}


def plain_knobs():
    """The reference launch: never packed, the default schedule."""
    ca.narrow_pack(0)
    ca.kseg_schedule(0, 0)


def form_knobs(sched):
    """The form's launch: packed where the library packs by default (NPROMA <= 16), the schedule under test."""
    ca.narrow_pack(-1)
    ca.kseg_schedule(*sched)


# ---------------------------------------------------------------------------
# outputs in the template's layout against a reference (tests/test_gpu_parity.py, tests/test_gpu_api.py)
# ---------------------------------------------------------------------------
RELL1_FP32_FAST = 1e-4


def rel_l1(a, r):
    a = np.asarray(a, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    den = np.abs(r).sum()
    num = np.abs(a - r).sum()
    return num / den if den > 0 else num


def field_report(out, ref):
    rep = {}
    for _, k in ca.VALIDATED:
        a, r = out[k], ref[k]
        assert a.shape == r.shape, (k, a.shape, r.shape)
        assert np.all(np.isfinite(a)), k
        d = np.abs(a.astype(np.float64) - r.astype(np.float64))
        mref = float(np.abs(r).max())
        rep[k] = (rel_l1(a, r), float(d.max()), mref)
    return rep


def oracle_outputs(oracle_mod, ds, ngptot, nproma, precision=ca.FP64):
    st, _ = oracle_mod.run_oracle(ds, ngptot, nproma, precision)
    return ca.state_outputs_to_template(st.arrays, ngptot)


def bitwise_mismatches(out, ref):
    bad = {}
    for _, k in ca.VALIDATED:
        n = int(np.count_nonzero(widened_bits(out[k]) != widened_bits(ref[k])))
        if n:
            bad[k] = (n, rel_l1(out[k], ref[k]))
    return bad


def fp32_gates(out, ref, gold, cpu_vs_gold):
    """relL1 <= 1e-4 per field vs the fp32 restatement, and vs reference.h5 no
    worse than 2x the fp32 restatement's own error plus a floor."""
    rep = field_report(out, ref)
    for k, v in sorted(rep.items(), key=lambda kv: -kv[1][0])[:6]:
        print("fp32 fast libm vs fp32 restatement %-18s relL1 %.3e" % (k, v[0]))
    bad = {k: v[0] for k, v in rep.items() if not v[0] <= RELL1_FP32_FAST}
    assert bad == {}, bad
    g = field_report(out, gold)
    for k in g:
        assert g[k][0] <= 2.0 * cpu_vs_gold[k][0] + 1e-6, (k, g[k][0], cpu_vs_gold[k][0])
