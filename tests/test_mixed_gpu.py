"""CLOUDSC_MIXED on the device: float fields, double arithmetic.  Everything is
compared on raw bits (view(uint32)) over the 20 outputs and plude against

    expected = float32( oracle_fp64( float64( float32(inputs) ) ) )

(tests/mixed_expected.py: the unchanged fp64 restatement; never the kernel
under test)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cloudsc_amd as ca
import mixed_expected as mx
from gpu_harness import init_params, kseg_workspace, lib, uses_aerosols  # noqa: F401  (lib: fixture)
from host_harness import configured

pytestmark = pytest.mark.gpu


@pytest.fixture
def default_schedule():
    yield
    ca.kseg_schedule(0, 0)


def device_run(lib, ds, ngptot, nproma, variant, schedules=((0, 0),), precision=ca.MIXED):
    """cloudsc_gpu_run on caller-owned buffers (DeviceFields), plude restored
    before every launch; yields the outputs of each schedule.  KSEG runs on a
    workspace of cloudsc_gpu_scratch_bytes and is followed by cloudsc_gpu_check."""
    df = ca.DeviceFields(ngptot, nproma, ds.klev, precision, place=False, aerosols=uses_aerosols(ds))
    hip = ca._hip()
    ws = C.c_void_p()
    outs = []
    try:
        st = ca.make_host_state(ds, ngptot, nproma, precision)
        ins = {k: v for k, v in st.arrays.items() if k not in ca.OUTPUT_FIELDS}
        init_params(lib, ds.params)
        ws = kseg_workspace(lib, hip, precision, variant, ngptot, nproma, ds.klev)
        for nseg, grid in schedules:
            df.upload(ins)
            ca.kseg_schedule(nseg, grid)
            ca.check(lib.cloudsc_gpu_run(0, None, precision, variant, ngptot, nproma, ds.klev, C.byref(df.f), ws))
            assert lib.cloudsc_gpu_check(0, None, variant, ws) == 0
            outs.append({k: ca.blocks_to_columns(df.download(k), ngptot) for _, k in ca.VALIDATED})
    finally:
        ca.kseg_schedule(0, 0)
        if ws.value:
            hip.hipFree(ws)
        df.close()
    return outs


# ---------------------------------------------------------------------------
# the kernels through cloudsc_gpu_run
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ngptot", [100, 130])
@pytest.mark.parametrize("nproma", [1, 33, 64, 100, 128, 256])
def test_kcache_mixed_bitwise(lib, ds, oracle_mod, ngptot, nproma):
    exp = mx.expected(oracle_mod, ds, ngptot, nproma, key="ref100")
    out, = device_run(lib, ds, ngptot, nproma, ca.VARIANT_KCACHE)
    assert mx.mismatches(out, exp) == {}


# default schedule, then 1, 2 and 3 segments on grids of 1 and 3 workgroups
KSEG_SCHEDULES = ((0, 0), (1, 1), (1, 3), (2, 1), (2, 3), (3, 1), (3, 3))


@pytest.mark.parametrize("nproma,ngptot", [(16, 130), (64, 130), (128, 300), (300, 300)])
def test_kseg_mixed_bitwise_schedules(lib, ds, oracle_mod, default_schedule, nproma, ngptot):
    """Segment hand-offs (the carried state stays double in the workspace) and
    several 64-column sub-blocks per block, one wide block included."""
    exp = mx.expected(oracle_mod, ds, ngptot, nproma, key="ref100")
    outs = device_run(lib, ds, ngptot, nproma, ca.VARIANT_KSEG, KSEG_SCHEDULES)
    for sched, out in zip(KSEG_SCHEDULES, outs):
        assert mx.mismatches(out, exp) == {}, sched


# ---------------------------------------------------------------------------
# state API
# ---------------------------------------------------------------------------
def test_state_api_mixed(lib, ds, oracle_mod):
    """1000 columns / NPROMA 128 through cloudsc_state_*: KSEG == KCACHE ==
    expected, repeated steps give the same bits (plude out of place), the
    download widens exactly, and the on-device statistics are those of the
    downloaded arrays."""
    n, nproma = 1000, 128
    exp = mx.expected(oracle_mod, ds, n, nproma, key="ref100")
    g = ca.GpuState(ds, n, nproma, ca.MIXED)
    try:
        g.run(ca.VARIANT_KSEG, 1)
        kseg = g.outputs()
        g.run(ca.VARIANT_KSEG, 3)
        kseg3 = g.outputs()
        dev = g.validate()
        g.run(ca.VARIANT_KCACHE, 1)
        kcache = g.outputs()
        fields = ca.Fields()
        ca.check(lib.cloudsc_state_fields(g.h, C.byref(fields)))
        assert fields.pt and fields.plude and fields.pfplsn
        idx = [k for _, k in ca.VALIDATED].index("tendency_loc_cld")
        assert lib.cloudsc_state_field_elems(g.h, idx) == ca.nblocks_of(n, nproma) * 5 * ds.klev * nproma
    finally:
        g.close()
    for out in (kseg, kseg3, kcache):       # as_f32 asserts every double holds a float value
        assert mx.mismatches(out, exp) == {}
    tiled = {k: np.take(ds.reference[k], np.arange(n) % ds.klon, axis=-1) for _, k in ca.VALIDATED}
    for i, (_, k) in enumerate(ca.VALIDATED):
        host = ca.field_stats(kseg3[k], tiled[k])
        for a, b in zip(dev[i], host):
            assert a == pytest.approx(b, rel=1e-12, abs=1e-300), (k, dev[i], host)


def test_interleaved_fp64_and_mixed_states(lib, ds, oracle_mod):
    """An fp64 state and a mixed state with different NSSOPT on one device,
    run interleaved: each matches its own expectation."""
    s0 = ds.copy()
    s0.params = dict(s0.params)
    s0.params["nssopt"] = 0
    n, nproma = 1000, 128
    a = ca.GpuState(ds, n, nproma, ca.FP64)
    b = ca.GpuState(s0, n, nproma, ca.MIXED)
    try:
        a.run(ca.VARIANT_KSEG, 1)
        b.run(ca.VARIANT_KSEG, 1)
        a.run(ca.VARIANT_KCACHE, 1)
        out_b = b.outputs()
        out_a = a.outputs()
    finally:
        a.close()
        b.close()
    assert mx.mismatches(out_b, mx.expected(oracle_mod, s0, n, nproma, key="nssopt0")) == {}
    ref, _ = oracle_mod.run_oracle(ds, n, nproma)
    for _, k in ca.VALIDATED:
        r = ca.blocks_to_columns(ref.arrays[k], n)
        assert np.array_equal(np.ascontiguousarray(out_a[k]).view(np.uint64), r.view(np.uint64)), k


# ---------------------------------------------------------------------------
# regimes and edges
# ---------------------------------------------------------------------------
# Input edges (make_fixtures.EDGE_CASES).  Determined on the CPU: in all ten
# the float-rounded inputs are finite and the fp64 restatement's outputs on
# them are finite, so none is left out.  In condensate_1e-200 and
# condensate_subnormal every condensate input rounds to zero in float (9677
# elements): they run as a second no-condensate state.
EDGES = ("condensate_1e-200", "condensate_subnormal", "condensate_x1000", "no_water", "full_cover", "hot_plus60K",
         "cold_minus80K", "tendencies_x100", "pressure_x0.01", "mass_flux_x100")
REGIMES = ("ref100", "cold", "dry", "moist", "seed1", "seed2", "aerosol", "nssopt2", "nssopt3", "ncldtop2",
           "ncldtop138", "klev3", "klev16")
PARAM_EDGES = ("ptsphy_60", "ptsphy_900", "ptsphy_1234.567", "ptsphy_7200", "tuning_jitter_1", "tuning_jitter_2")


def case_state(ds, case):
    import make_fixtures as mf
    if case == "ref100":
        return ds
    if case in EDGES:
        return mf.edge_case(ds, case)
    if case in PARAM_EDGES:
        return mf.param_case(ds, case)
    if case == "tiny_condensate":
        # condensate inputs scaled into the float subnormal range: outputs that
        # are non-zero float subnormals (36281 of them on the CPU at this shape)
        s = ds.copy()
        for k in ("pclv", "tendency_tmp_cld", "plude"):
            s.inputs[k] = s.inputs[k] * 1e-35
        s.reference = {}
        return s
    return configured(ds, case)


@pytest.mark.parametrize("case", REGIMES + PARAM_EDGES + EDGES + ("tiny_condensate",))
def test_mixed_regimes_and_edges(lib, ds, oracle_mod, case):
    import make_fixtures as mf
    assert set(EDGES) == set(mf.EDGE_CASES) and set(PARAM_EDGES) == set(mf.PARAM_CASES)
    s = case_state(ds, case)
    exp = mx.expected(oracle_mod, s, 130, 64, key=case)
    assert mx.all_finite(exp)
    kseg, = device_run(lib, s, 130, 64, ca.VARIANT_KSEG)
    assert mx.mismatches(kseg, exp) == {}
    kcache, = device_run(lib, s, 130, 64, ca.VARIANT_KCACHE)
    assert mx.mismatches(kcache, exp) == {}


def test_mixed_store_keeps_subnormals(lib, ds, oracle_mod):
    """The narrowing store underflows gradually: the compared outputs hold
    non-zero float subnormals, so a flush-to-zero store cannot pass."""
    s = case_state(ds, "tiny_condensate")
    exp = mx.expected(oracle_mod, s, 130, 64, key="tiny_condensate")
    n = mx.subnormal_count(exp)
    print("non-zero float subnormals among the compared outputs:", n)
    assert n > 0
    out, = device_run(lib, s, 130, 64, ca.VARIANT_KSEG)
    assert mx.subnormal_count({k: mx.as_f32(v) for k, v in out.items()}) == n
    assert mx.mismatches(out, exp) == {}


# ---------------------------------------------------------------------------
# accuracy against reference.h5
# ---------------------------------------------------------------------------
def test_mixed_accuracy_vs_reference_h5(lib, ds, oracle_mod):
    """Per field, the mixed relL1 against reference.h5 (cloudsc_state_validate)
    is within 2x that of `expected` (the restatement, computed on the CPU) plus
    the floor of the fp32 gate, 1e-6."""
    n, nproma = 1000, 128
    exp = mx.expected(oracle_mod, ds, n, nproma, key="ref100")
    gold = {k: np.take(ds.reference[k], np.arange(n) % ds.klon, axis=-1) for _, k in ca.VALIDATED}
    cpu = mx.rel_l1(exp, gold)
    g = ca.GpuState(ds, n, nproma, ca.MIXED)
    try:
        g.run(ca.VARIANT_KSEG, 1)
        stats = g.validate()
    finally:
        g.close()
    for (name, k), st in zip(ca.VALIDATED, stats):
        rel = ca.rel_error(st[3], st[4])[0]
        print("mixed vs reference.h5 %-18s relL1 gpu %.3e expected %.3e" % (k, rel, cpu[k]))
        assert rel <= 2.0 * cpu[k] + 1e-6, (name, rel, cpu[k])


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_mixed_refusals_then_fp64(lib, ds, oracle_mod):
    """No mixed form of SCC / SCC_PRIVATE, the host pipeline or cloudsc_host_run:
    CLOUDSC_EINVAL, and a correct fp64 run follows in the same process."""
    n, nproma = 130, 64
    p = ca.Params.from_dict(ds.params)
    ca.check(lib.cloudsc_gpu_init(0, C.byref(p)))
    df = ca.DeviceFields(n, nproma, ds.klev, ca.MIXED, place=False)
    try:
        for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE):
            assert lib.cloudsc_gpu_run(0, None, ca.MIXED, variant, n, nproma, ds.klev, C.byref(df.f),
                                       df.f.pt) == ca.EINVAL
            assert lib.cloudsc_gpu_scratch_bytes(ca.MIXED, variant, n, nproma, ds.klev) <= 0
    finally:
        df.close()
    g = ca.GpuState(ds, n, nproma, ca.MIXED)
    try:
        for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE):
            assert lib.cloudsc_state_run(g.h, variant, 1, None) == ca.EINVAL
    finally:
        g.close()
    st = ca.make_host_state(ds, n, nproma, ca.MIXED)
    f = st.fields()
    h = C.c_void_p()
    assert lib.cloudsc_host_pipeline_create(C.byref(h), 0, ca.MIXED, n, nproma, ds.klev, 2, 2, C.byref(f)) == ca.EINVAL
    assert not h.value
    lib.cloudsc_host_run.argtypes = [C.c_int] * 6 + [C.POINTER(ca.Params), C.POINTER(ca.Fields)]
    assert lib.cloudsc_host_run(0, ca.MIXED, ca.VARIANT_KSEG, n, nproma, ds.klev, C.byref(p), C.byref(f)) == ca.EINVAL
    out, = device_run(lib, ds, n, nproma, ca.VARIANT_KSEG, precision=ca.FP64)
    ref, _ = oracle_mod.run_oracle(ds, n, nproma)
    for _, k in ca.VALIDATED:
        r = ca.blocks_to_columns(ref.arrays[k], n)
        assert np.array_equal(np.ascontiguousarray(out[k]).view(np.uint64), r.view(np.uint64)), k


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------
def cli_rows(stdout):
    return [l for l in stdout.splitlines() if re.match(r"\s+\S+ \dD\d ", l)]


def test_dwarf_cli_mixed(lib, ds):
    """`dwarf-cloudsc-amd 1 1000 64 --precision mixed`: reported like fp32 (no
    gate without --tol, exit status 0; with --tol the gate decides), the error
    column is that of the Python statistics, and --gpus 2 prints the same table."""
    exe = os.path.join(os.path.dirname(ca.LIB_PATH), "dwarf-cloudsc-amd")
    run = lambda *a: subprocess.run([exe, "1", "1000", "64", "--precision", "mixed"] + list(a),
                                    capture_output=True, text=True, timeout=120)
    r = run()
    print(r.stdout[-3000:], r.stderr[-1000:])
    assert r.returncode == 0
    assert "CLOUDSC-AMD: mixed, variant kseg" in r.stdout
    assert "VALIDATION: reported only (mixed vs the fp64 reference" in r.stdout
    rows = cli_rows(r.stdout)
    assert len(rows) == 21
    g = ca.GpuState(ds, 1000, 64, ca.MIXED)
    try:
        g.run(ca.VARIANT_KSEG, 1)
        stats = g.validate()
    finally:
        g.close()
    for (name, k), st, row in zip(ca.VALIDATED, stats, rows):
        cols = row.split()       # name, dims, min, max, max|d|, avg|d| per column, relative error in %
        rel = ca.rel_error(st[3], st[4])[0]
        assert float(cols[6]) == pytest.approx(100.0 * rel, rel=1e-11, abs=1e-300), (row, rel)
        assert float(cols[4]) == pytest.approx(st[2], rel=1e-11, abs=1e-300), (row, st)
        assert float(cols[5]) == pytest.approx(st[3] / 1000, rel=1e-11, abs=1e-300), (row, st)
    r2 = run("--gpus", "2")
    assert r2.returncode == 0 and cli_rows(r2.stdout) == rows
    assert run("--tol", "1e-30").returncode != 0 and run("--tol", "1.0").returncode == 0
    assert run("--variant", "scc").returncode != 0
