"""GPU parity tests: the HIP kernels (through the libcloudsc_amd.so C ABI) against
the oracle (C restatement, itself bit-exact vs the reference C kernel) and the
reference goldens (data/reference_*.dat == config-files/reference.h5).

fp64 is compared BIT FOR BIT (the bitwise_* tests at the end): the kernels
keep the reference's operation order with no FMA contraction
(-ffp-contract=off), divide with correct rounding, and evaluate exp/pow with
the reference CPU build's own algorithms (csrc/cloudsc_libm.h).  The tolerance
gates (relL1 <= 1e-12 per field, max|d| <= 1e-10 * max|ref|) remain for the
wider shape/variant matrix; SURVEY.md §8c measured that ulp-level exp/pow
perturbations move this kernel by relL1 ~2e-14.
fp32: vs the fp32 CPU restatement relL1 <= 1e-3 per field (the algorithm has
thresholds at 1e-14 / 1e-8 that float rounding crosses).
"""
import numpy as np
import pytest

import cloudsc_amd as ca
from gpu_harness import RELL1_FP32_FAST, bitwise_mismatches, field_report, fp32_gates, oracle_outputs, rel_l1  # noqa: F401
from gpu_harness import lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

RELL1_FP64 = 1e-12
MAXREL_FP64 = 1e-10
RELL1_FP32_VS_SP_ORACLE = 1e-3


def assert_close(rep, rell1, maxrel, label):
    bad = []
    for k, (rl, md, mref) in rep.items():
        lim = maxrel * mref if mref > 0 else 0.0
        if not (rl <= rell1 and md <= lim):
            bad.append("%s: relL1=%.3e maxabs=%.3e (max|ref|=%.3e)" % (k, rl, md, mref))
    worst = max(rep.items(), key=lambda kv: kv[1][0])
    print("[%s] worst relL1 %s = %.3e" % (label, worst[0], worst[1][0]))
    assert not bad, "%s: fields out of tolerance:\n  " % label + "\n  ".join(bad)


def run_gpu(ds, ngptot, nproma, precision=ca.FP64, variant=ca.VARIANT_KCACHE, col_offset=0):
    g = ca.GpuState(ds, ngptot, nproma, precision, col_offset=col_offset)
    try:
        g.run(variant, 1)
        return g.outputs()
    finally:
        g.close()


@pytest.mark.parametrize("nproma", [100, 128, 64])
def test_kcache_vs_oracle_100(lib, ds, oracle_mod, nproma):
    out = run_gpu(ds, 100, nproma)
    ref = oracle_outputs(oracle_mod, ds, 100, nproma)
    assert_close(field_report(out, ref), RELL1_FP64, MAXREL_FP64, "kcache vs oracle nproma=%d" % nproma)


def test_kcache_vs_golden(lib, ds):
    out = run_gpu(ds, 100, 128)
    gold = {k: ds.reference[k] for _, k in ca.VALIDATED}
    rep = field_report(out, gold)
    # the oracle itself differs from the Fortran-generated goldens by <= 5e-17 relL1
    assert_close(rep, RELL1_FP64, MAXREL_FP64, "kcache vs reference.h5")


@pytest.mark.parametrize("name", ["W", "M"])
def test_kcache_scenarios(lib, scenarios, name):
    s = scenarios[name]
    out = run_gpu(s, 100, 128)
    assert_close(field_report(out, s.reference), RELL1_FP64, MAXREL_FP64, "kcache scenario %s" % name)


def test_partial_last_block(lib, ds, oracle_mod):
    # the reference GPU ctest shape: 1 1000 128 (1000 = 7*128 + 104)
    out = run_gpu(ds, 1000, 128)
    ref = oracle_outputs(oracle_mod, ds, 1000, 128)
    assert_close(field_report(out, ref), RELL1_FP64, MAXREL_FP64, "1000/128")


def test_nproma_invariance_bitwise(lib, ds):
    a = run_gpu(ds, 1000, 128)
    for nproma in (64, 256, 100):
        b = run_gpu(ds, 1000, nproma)
        for _, k in ca.VALIDATED:
            assert np.array_equal(a[k], b[k]), (nproma, k)


def test_replica_invariance_bitwise(lib, ds):
    # global column g uses template column g % 100, so columns g and g+100 are
    # the same problem and must give bit-identical results
    out = run_gpu(ds, 1000, 128)
    for _, k in ca.VALIDATED:
        x = out[k].reshape(-1, 1000)
        for r in range(1, 10):
            assert np.array_equal(x[:, :100], x[:, 100 * r:100 * (r + 1)]), k


def test_scc_equals_kcache_bitwise(lib, ds):
    a = run_gpu(ds, 1000, 128, variant=ca.VARIANT_KCACHE)
    b = run_gpu(ds, 1000, 128, variant=ca.VARIANT_SCC)
    for _, k in ca.VALIDATED:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["W", "M"])
def test_scc_scenarios(lib, scenarios, name):
    s = scenarios[name]
    out = run_gpu(s, 100, 128, variant=ca.VARIANT_SCC)
    assert_close(field_report(out, s.reference), RELL1_FP64, MAXREL_FP64, "scc scenario %s" % name)


# ---- SCC with per-thread private-array temporaries (the reference's cloudsc_c.cu form, a3) ----
@pytest.mark.parametrize("precision", [ca.FP64, ca.FP32])
def test_scc_private_equals_kcache_bitwise(lib, ds, precision):
    a = run_gpu(ds, 1000, 128, precision=precision, variant=ca.VARIANT_KCACHE)
    b = run_gpu(ds, 1000, 128, precision=precision, variant=ca.VARIANT_SCC_PRIVATE)
    for _, k in ca.VALIDATED:
        assert np.array_equal(a[k], b[k]), k


def gpu_init_default(lib, ds, device=0):
    """cloudsc_gpu_init: the device's default parameter set, which the
    low-level cloudsc_gpu_run reads (each test sets it itself, so it passes
    alone)."""
    import ctypes as C
    prm = ca.Params.from_dict(ds.params)
    ca.check(lib.cloudsc_gpu_init(device, C.byref(prm)))


def test_scc_private_klev_bound(lib, ds):
    """The private arrays are sized for the reference's klev = 137: more levels is EINVAL."""
    import ctypes as C
    gpu_init_default(lib, ds)
    g = ca.GpuState(ds, 256, 128)
    try:
        f = ca.Fields()
        ca.check(lib.cloudsc_state_fields(g.h, C.byref(f)))
        assert lib.cloudsc_gpu_run(0, None, ca.FP64, ca.VARIANT_SCC_PRIVATE, 256, 128, 138, C.byref(f), None) == -1
        ca.check(lib.cloudsc_state_sync(g.h))
    finally:
        g.close()


def test_shard_offset_bitwise(lib, ds):
    # a shard starting at global column 384 reproduces the tail of the full run
    full = run_gpu(ds, 1024, 128)
    shard = run_gpu(ds, 640, 128, col_offset=384)
    for _, k in ca.VALIDATED:
        assert np.array_equal(full[k][..., 384:], shard[k]), k


def test_fp32_vs_fp32_oracle(lib, ds, oracle_mod):
    out = run_gpu(ds, 1000, 128, precision=ca.FP32)
    ref = oracle_outputs(oracle_mod, ds, 1000, 128, precision=ca.FP32)
    rep = field_report(out, ref)
    bad = [(k, v) for k, v in rep.items() if v[0] > RELL1_FP32_VS_SP_ORACLE]
    for k, v in sorted(rep.items(), key=lambda kv: -kv[1][0])[:5]:
        print("fp32 gpu vs fp32 oracle %-18s relL1 %.3e" % (k, v[0]))
    assert not bad, bad


def test_fp32_vs_fp64_reference_reported(lib, ds, oracle_mod):
    # fp32 vs the fp64 goldens: the GPU fp32 path must not be worse than 2x the
    # fp32 CPU restatement (plus a floor) on any field (SURVEY.md §8c gate)
    out = run_gpu(ds, 100, 100, precision=ca.FP32)
    cpu = oracle_outputs(oracle_mod, ds, 100, 100, precision=ca.FP32)
    gold = {k: ds.reference[k] for _, k in ca.VALIDATED}
    g = field_report(out, gold)
    c = field_report(cpu, gold)
    for k in g:
        assert g[k][0] <= 2.0 * c[k][0] + 1e-6, (k, g[k][0], c[k][0])


def test_device_validation_matches_host(lib, ds):
    g = ca.GpuState(ds, 1000, 128)
    try:
        g.run(ca.VARIANT_KCACHE, 1)
        dev = g.validate()
        out = g.outputs()
    finally:
        g.close()
    tiled = {k: np.take(ds.reference[k], np.arange(1000) % 100, axis=-1) for _, k in ca.VALIDATED}
    for i, (_, k) in enumerate(ca.VALIDATED):
        host = ca.field_stats(out[k], tiled[k])
        for a, b in zip(dev[i], host):
            assert a == pytest.approx(b, rel=1e-12, abs=1e-300), (k, dev[i], host)


def test_full_size_validation(lib, ds):
    """BASELINE size (163840 columns, NPROMA 128): every field within the gate
    against reference.h5 replicated with g % 100, computed on the device."""
    g = ca.GpuState(ds, 163840, 128)
    try:
        g.run(ca.VARIANT_KCACHE, 1)
        stats = g.validate()
        plude = g.download("plude")
        tlt = g.download("tendency_loc_t")
    finally:
        g.close()
    for (name, k), (mn, mx, maxerr, errsum, refsum) in zip(ca.VALIDATED, (st[:5] for st in stats)):
        rel = errsum / refsum if refsum > 0 else errsum
        assert rel <= RELL1_FP64, (name, rel)
        assert np.isfinite(mn) and np.isfinite(mx)
    # replica invariance at full size: block b, lane l is column b*128+l
    for f in (plude, tlt):
        cols = ca.blocks_to_columns(f, 163840)
        assert np.array_equal(cols[:, :100], cols[:, 163700:163800])


def test_low_level_run_entry(lib, ds):
    """cloudsc_gpu_run on caller-owned device buffers (the drop-in boundary)."""
    import ctypes as C
    gpu_init_default(lib, ds)
    g = ca.GpuState(ds, 256, 128)
    try:
        f = ca.Fields()
        ca.check(lib.cloudsc_state_fields(g.h, C.byref(f)))
        ca.check(lib.cloudsc_state_reset(g.h))
        ca.check(lib.cloudsc_state_sync(g.h))
        ca.check(lib.cloudsc_gpu_run(0, None, ca.FP64, ca.VARIANT_KCACHE, 256, 128, ds.klev, C.byref(f), None))
        ca.check(lib.cloudsc_state_sync(g.h))
        import ctypes
        assert lib.cloudsc_gpu_run(0, None, ca.FP64, ca.VARIANT_SCC, 256, 128, ds.klev, C.byref(f), None) == -1
        assert lib.cloudsc_gpu_run(0, None, 3, ca.VARIANT_KCACHE, 256, 128, ds.klev, C.byref(f), None) == -1
        assert lib.cloudsc_gpu_run(0, None, ca.FP64, ca.VARIANT_KCACHE, 256, 512, ds.klev, C.byref(f), None) == -1
        assert lib.cloudsc_gpu_run(999, None, ca.FP64, ca.VARIANT_KCACHE, 256, 128, ds.klev, C.byref(f), None) == -2
        out = g.outputs()
    finally:
        g.close()
    ref = run_gpu(ds, 256, 128)
    for _, k in ca.VALIDATED:
        assert np.array_equal(out[k], ref[k]), k


# ---- persistent segmented k-caching (KSEG): must be bit-identical to KCACHE ----
@pytest.fixture
def kseg_env():
    """Override the KSEG schedule (segments per column, grid) through the
    library's diagnostic setter; restored to the defaults afterwards."""
    def set_sched(nseg=None, grid=None):
        ca.kseg_schedule(nseg or 0, grid or 0)
    yield set_sched
    ca.kseg_schedule(0, 0)


@pytest.mark.parametrize("nseg,grid", [(1, None), (2, None), (4, None), (8, None), (4, 3), (8, 1), (3, 5)])
def test_kseg_equals_kcache_bitwise(lib, ds, kseg_env, nseg, grid):
    # grid 1 / 3 / 5: few workgroups, so most segments wait on a predecessor
    # that another (or the same) workgroup finished earlier
    a = run_gpu(ds, 1000, 128, variant=ca.VARIANT_KCACHE)
    kseg_env(nseg, grid)
    b = run_gpu(ds, 1000, 128, variant=ca.VARIANT_KSEG)
    for _, k in ca.VALIDATED:
        assert np.array_equal(a[k], b[k]), (nseg, grid, k)


@pytest.mark.parametrize("name", ["W", "M"])
def test_kseg_scenarios(lib, scenarios, kseg_env, name):
    s = scenarios[name]
    kseg_env(4, None)
    out = run_gpu(s, 100, 128, variant=ca.VARIANT_KSEG)
    assert_close(field_report(out, s.reference), RELL1_FP64, MAXREL_FP64, "kseg scenario %s" % name)


def test_kseg_fp32_equals_kcache_bitwise(lib, ds, kseg_env):
    a = run_gpu(ds, 1000, 128, precision=ca.FP32, variant=ca.VARIANT_KCACHE)
    kseg_env(4, 7)
    b = run_gpu(ds, 1000, 128, precision=ca.FP32, variant=ca.VARIANT_KSEG)
    for _, k in ca.VALIDATED:
        assert np.array_equal(a[k], b[k]), k


def test_kseg_full_size(lib, ds, kseg_env):
    """BASELINE size with the default segmentation and grid: bit-identical to
    KCACHE on every validated field, repeated launches reuse the workspace."""
    kseg_env(None, None)
    g = ca.GpuState(ds, 163840, 128)
    try:
        g.run(ca.VARIANT_KCACHE, 1)
        a = {k: g.download(k) for _, k in ca.VALIDATED}
        g.run(ca.VARIANT_KSEG, 3)
        for _, k in ca.VALIDATED:
            assert np.array_equal(a[k], g.download(k)), k
    finally:
        g.close()


# ---- branch coverage beyond the shipped state (same cases the oracle is pinned on) ----
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("variant", [ca.VARIANT_KCACHE, ca.VARIANT_KSEG])
def test_random_perturbations_vs_oracle(lib, ds, oracle_mod, seed, variant):
    import make_fixtures as mf
    s = mf.perturbed(ds, seed)
    out = run_gpu(s, 1000, 128, variant=variant)
    ref = oracle_outputs(oracle_mod, s, 1000, 128)
    assert_close(field_report(out, ref), RELL1_FP64, MAXREL_FP64, "perturbed seed %d" % seed)


@pytest.mark.parametrize("nssopt", [0, 2, 3])
@pytest.mark.parametrize("variant", [ca.VARIANT_KCACHE, ca.VARIANT_SCC_PRIVATE])
def test_nssopt_vs_oracle(lib, ds, oracle_mod, nssopt, variant):
    s = ds.copy()
    s.params["nssopt"] = nssopt
    out = run_gpu(s, 300, 128, variant=variant)
    ref = oracle_outputs(oracle_mod, s, 300, 128)
    assert_close(field_report(out, ref), RELL1_FP64, MAXREL_FP64, "nssopt %d" % nssopt)


@pytest.mark.parametrize("variant", [ca.VARIANT_KCACHE, ca.VARIANT_KSEG, ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE])
def test_aerosol_flags_vs_oracle(lib, ds, oracle_mod, variant):
    import make_fixtures as mf
    s = mf.with_aerosols(ds)
    out = run_gpu(s, 300, 128, variant=variant)
    ref = oracle_outputs(oracle_mod, s, 300, 128)
    assert_close(field_report(out, ref), RELL1_FP64, MAXREL_FP64, "aerosol flags")


# ---- host-buffer pipeline (H2D -> kernel -> D2H, chunked over streams) ----
@pytest.mark.parametrize("variant,chunk,nstreams", [(ca.VARIANT_KCACHE, 3, 2), (ca.VARIANT_KSEG, 2, 3),
                                                     (ca.VARIANT_SCC, 5, 1), (ca.VARIANT_KCACHE, 100, 4),
                                                     (ca.VARIANT_SCC_PRIVATE, 3, 2)])
def test_host_pipeline_equals_resident(lib, ds, variant, chunk, nstreams):
    """Chunks of a few blocks (the last one partial, with the partial last
    block) give the same bits as the device-resident run."""
    ref = run_gpu(ds, 1000, 128, variant=ca.VARIANT_KCACHE)
    hp = ca.HostPipeline(ds, 1000, 128, chunk_blocks=chunk, nstreams=nstreams)
    try:
        hp.run(variant)
        hp.run(variant)                     # plude restored between steps
        out = hp.outputs()
    finally:
        hp.close()
    for _, k in ca.VALIDATED:
        assert np.array_equal(out[k], ref[k]), k


@pytest.mark.parametrize("variant", [ca.VARIANT_SCC, ca.VARIANT_KSEG, ca.VARIANT_KCACHE])
def test_host_pipeline_packed_arrays(lib, ds, variant):
    """Host arrays carved back to back out of one buffer, so that neighbouring
    fields share pages: the pipeline pins merged page ranges, every array lies
    inside one registration, and the chunked run gives the resident bits.
    (Pinning each array on its own faulted the device in round 2.)"""
    ref = run_gpu(ds, 1000, 128, variant=ca.VARIANT_KCACHE)
    hp = ca.HostPipeline(ds, 1000, 128, chunk_blocks=5, nstreams=1, packed=True)
    try:
        # the invariant whose violation faulted: every array resolves, from its
        # first to its last byte, as ONE pinned mapping
        n, bad = hp.mapping()
        assert n >= 40 and bad == 0, (n, bad)
        arrays = hp.host_arrays()
        assert all(lib.cloudsc_debug_host_pinned(p, nb) == 1 for p, nb in arrays)
        hp.run(variant)
        hp.run(variant)
        out = hp.outputs()
    finally:
        hp.close()
    # destroy leaves no registration behind (the buffer itself is still alive)
    assert [p for p, nb in arrays if lib.cloudsc_debug_host_pinned(p, nb) != 0] == []
    for _, k in ca.VALIDATED:
        assert np.array_equal(out[k], ref[k]), k


def test_host_pipeline_fp32(lib, ds):
    ref = run_gpu(ds, 1000, 128, precision=ca.FP32)
    hp = ca.HostPipeline(ds, 1000, 128, precision=ca.FP32, chunk_blocks=4, nstreams=2)
    try:
        hp.run(ca.VARIANT_KCACHE)
        out = hp.outputs()
    finally:
        hp.close()
    for _, k in ca.VALIDATED:
        assert np.array_equal(out[k], ref[k]), k


@pytest.mark.parametrize("variant,nstreams", [(ca.VARIANT_KSEG, 3), (ca.VARIANT_KCACHE, 3), (ca.VARIANT_KSEG, 1),
                                              (ca.VARIANT_KCACHE, 2)])
def test_host_pipeline_copy_paths(lib, ds, variant, nstreams):
    """Every copy path of the pipeline (cloudsc_debug_set_pipeline_copy: copy
    engines pinned per direction -- the default --, HIP streams, HIP streams
    with a copy kernel for the outputs) gives the resident bits, over chunks
    whose slots are reused (8 chunks on 1-3 slots, the last one partial).  The
    default path runs on two different engines, whose overlap it measured at
    creation.  With one or two slots the H2D of plude (INOUT) into a reused
    slot must wait for the D2H that reads the previous chunk's plude back out
    of it: with one slot that D2H is the previous chunk's own."""
    ref = run_gpu(ds, 1000, 64, variant=ca.VARIANT_KCACHE)
    assert lib.cloudsc_debug_set_pipeline_copy(3) == ca.EINVAL
    try:
        for mode in (1, 0, 2):
            ca.check(lib.cloudsc_debug_set_pipeline_copy(mode))
            hp = ca.HostPipeline(ds, 1000, 64, chunk_blocks=2, nstreams=nstreams)
            try:
                m, e_in, e_out = hp.copy_path()
                if mode == 1:
                    assert m == 1 and e_in and e_out and e_in != e_out, (m, e_in, e_out)
                    # the engine pair check at creation measured the kept pair
                    overlap, pairs = hp.engine_check()
                    assert 1 <= pairs <= 6 and 0.5 < overlap < 2.5, (overlap, pairs)
                    # the copies-only bound runs on the same arrays; the steps below restore plude
                    assert hp.copy_bound() > 0.0
                hp.run(variant)
                hp.run(variant)
                out = hp.outputs()
            finally:
                hp.close()
            for _, k in ca.VALIDATED:
                assert np.array_equal(out[k], ref[k]), (mode, k)
    finally:
        ca.check(lib.cloudsc_debug_set_pipeline_copy(-1))


# ---- shapes beyond the reference's: other KLEV, tiny and ragged problems ----
def sliced_levels(ds, lo_lev):
    import make_fixtures as mf
    return mf.sliced_levels(ds, lo_lev)


@pytest.mark.parametrize("klev", [60, 3, 16, 274])
@pytest.mark.parametrize("variant", [ca.VARIANT_KCACHE, ca.VARIANT_KSEG, ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE])
def test_other_klev_vs_oracle(lib, ds, oracle_mod, variant, klev):
    """Shallow columns (the bottom 60, 16 or 3 levels; NCLDTOP 2 for the last
    two) and a deep one (274 levels: every layer split in two), bit for bit.
    SCC_PRIVATE's private arrays are sized for KLEV <= 137 (as the reference
    CUDA SCC kernel's): deeper columns are rejected."""
    import make_fixtures as mf
    if klev == 274:
        s = mf.refined_levels(ds, 2)
    else:
        s = sliced_levels(ds, ds.klev - klev)
        if klev < 60:
            s.params["ncldtop"] = 2
    if variant == ca.VARIANT_SCC_PRIVATE and klev > 137:
        with pytest.raises(ca.CloudscError):
            run_gpu(s, 300, 64, variant=variant)
        return
    out = run_gpu(s, 300, 64, variant=variant)
    ref = oracle_outputs(oracle_mod, s, 300, 64)
    assert bitwise_mismatches(out, ref) == {}


@pytest.mark.parametrize("ngptot,nproma", [(1, 1), (1, 64), (5, 256), (127, 64), (257, 256), (64, 32)])
@pytest.mark.parametrize("variant", [ca.VARIANT_KCACHE, ca.VARIANT_KSEG, ca.VARIANT_SCC_PRIVATE])
def test_tiny_and_ragged(lib, ds, oracle_mod, ngptot, nproma, variant):
    out = run_gpu(ds, ngptot, nproma, variant=variant)
    ref = oracle_outputs(oracle_mod, ds, ngptot, nproma)
    for _, k in ca.VALIDATED:
        assert out[k].shape == ref[k].shape
    assert bitwise_mismatches(out, ref) == {}, (ngptot, nproma)


def test_invalid_arguments(lib, ds):
    import ctypes as C
    g = ca.GpuState(ds, 256, 64)
    try:
        f = ca.Fields()
        ca.check(lib.cloudsc_state_fields(g.h, C.byref(f)))
        args = (0, None, ca.FP64)
        assert lib.cloudsc_gpu_run(*args, 9, 256, 64, ds.klev, C.byref(f), None) == -1      # variant
        assert lib.cloudsc_gpu_run(*args, ca.VARIANT_KCACHE, 0, 64, ds.klev, C.byref(f), None) == -1
        assert lib.cloudsc_gpu_run(*args, ca.VARIANT_KCACHE, 256, 0, ds.klev, C.byref(f), None) == -1
        assert lib.cloudsc_gpu_run(*args, ca.VARIANT_KCACHE, 256, 64, 1, C.byref(f), None) == -1
        assert lib.cloudsc_gpu_run(*args, ca.VARIANT_KSEG, 256, 64, ds.klev, C.byref(f), None) == -1  # no ws
        f.pt = None
        assert lib.cloudsc_gpu_run(*args, ca.VARIANT_KCACHE, 256, 64, ds.klev, C.byref(f), None) == -1
        assert lib.cloudsc_state_run(g.h, 7, 1, None) == -1
        assert lib.cloudsc_state_run(g.h, ca.VARIANT_KCACHE, 0, None) == -1
        assert lib.cloudsc_state_download(g.h, 21, None) == -1
    finally:
        g.close()
    # parameters: NCLDTOP < 2 and NSSOPT out of range are rejected
    for key, val in (("ncldtop", 1), ("nssopt", 4), ("ptsphy", 0.0)):
        s = ds.copy()
        s.params[key] = val
        with pytest.raises(ca.CloudscError):
            ca.GpuState(s, 64, 64)


# ---- bit-for-bit parity with the reference kernel (fp64) ----
# The device exp/pow are the reference CPU build's own algorithms
# (csrc/cloudsc_libm.h, checked against the host C library by tests/test_libm.py),
# division is correctly rounded and no multiply-add is contracted, so the fp64
# GPU kernels reproduce the reference kernel (and its restatement, the oracle)
# bit for bit.  Scenario goldens W/M are the reference kernel's own outputs.
@pytest.mark.parametrize("variant", [ca.VARIANT_KCACHE, ca.VARIANT_KSEG, ca.VARIANT_SCC])
@pytest.mark.parametrize("ngptot,nproma", [(100, 128), (1000, 128), (1000, 64), (1000, 100), (1000, 256)])
def test_bitwise_vs_oracle(lib, ds, oracle_mod, variant, ngptot, nproma):
    # NPROMA 100 / 128 / 256: KSEG runs each block as 64-column one-wave items
    # (the last one of a block partial at NPROMA 100)
    out = run_gpu(ds, ngptot, nproma, variant=variant)
    ref = oracle_outputs(oracle_mod, ds, ngptot, nproma)
    assert bitwise_mismatches(out, ref) == {}


@pytest.mark.parametrize("ngptot,nproma", [(1000, 1000), (1000, 4096), (3000, 1000), (2048, 2048)])
def test_bitwise_kseg_wide_blocks(lib, ds, oracle_mod, ngptot, nproma):
    # KSEG accepts any NPROMA (KCACHE/SCC stop at 256 threads per block):
    # blocks wider than the columns, ragged sub-blocks, a partial last block,
    # and the level-major layout of a single block
    out = run_gpu(ds, ngptot, nproma, variant=ca.VARIANT_KSEG)
    ref = oracle_outputs(oracle_mod, ds, ngptot, nproma)
    assert bitwise_mismatches(out, ref) == {}


def test_wide_blocks_rejected_outside_kseg(lib, ds):
    import ctypes as C
    g = ca.GpuState(ds, 1024, 1024)
    try:
        f = ca.Fields()
        ca.check(lib.cloudsc_state_fields(g.h, C.byref(f)))
        for variant in (ca.VARIANT_KCACHE, ca.VARIANT_SCC):
            assert lib.cloudsc_gpu_run(0, None, ca.FP64, variant, 1024, 1024, ds.klev, C.byref(f), None) == -1
            assert lib.cloudsc_state_run(g.h, variant, 1, None) == -1
        ca.check(lib.cloudsc_state_run(g.h, ca.VARIANT_KSEG, 1, None))
    finally:
        g.close()


@pytest.mark.parametrize("name", ["W", "M"])
@pytest.mark.parametrize("variant", [ca.VARIANT_KCACHE, ca.VARIANT_KSEG, ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE])
def test_bitwise_vs_reference_kernel_scenarios(lib, scenarios, name, variant):
    s = scenarios[name]
    out = run_gpu(s, 100, 128, variant=variant)
    assert bitwise_mismatches(out, s.reference) == {}


def test_bitwise_vs_reference_kernel_built_here(lib, ds, oracle_mod):
    # the unmodified reference kernel, compiled from its own sources (oracle/_ref)
    if not oracle_mod.ref_available():
        pytest.skip("oracle/_ref not built (no reference checkout at build time)")
    st, _ = oracle_mod.run_ref(ds, 1000, 128)
    ref = ca.state_outputs_to_template(st.arrays, 1000)
    out = run_gpu(ds, 1000, 128, variant=ca.VARIANT_KSEG)
    assert bitwise_mismatches(out, ref) == {}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bitwise_random_perturbations(lib, ds, oracle_mod, seed):
    import make_fixtures as mf
    s = mf.perturbed(ds, seed)
    out = run_gpu(s, 1000, 128, variant=ca.VARIANT_KSEG)
    ref = oracle_outputs(oracle_mod, s, 1000, 128)
    assert bitwise_mismatches(out, ref) == {}


@pytest.mark.parametrize("case", ["nssopt0", "nssopt2", "nssopt3", "aerosol", "klev60", "divisor_params",
                                  "ncldtop2", "ncldtop40", "ncldtop120", "ncldtop137", "ncldtop138",
                                  "cold", "dry", "moist"])
def test_bitwise_other_configurations(lib, ds, oracle_mod, case):
    import make_fixtures as mf
    if case.startswith("ncldtop"):
        # the physics starts at NCLDTOP; KSEG's segment bounds follow it (kseg_bounds)
        s = ds.copy()
        s.params["ncldtop"] = int(case[len("ncldtop"):])
    elif case.startswith("nssopt"):
        s = ds.copy()
        s.params["nssopt"] = int(case[-1])
    elif case == "divisor_params":
        # the parameters the kernel divides by through host-folded reciprocals
        # (cl_div_known): other values with full mantissas, still the oracle's n/d
        s = ds.copy()
        for name, f in (("rtaumel", 0.7310432), ("rdepliqrefdepth", 1.913), ("rvrfactor", 1.3370001), ("rd", 1.0000137)):
            s.params[name] = s.params[name] * f
    elif case == "aerosol":
        s = mf.with_aerosols(ds)
    elif case in ("cold", "dry", "moist"):
        s = mf.shifted(ds, case)
    else:
        s = sliced_levels(ds, 77)
    ref = oracle_outputs(oracle_mod, s, 300, 64)
    variants = [ca.VARIANT_KSEG]
    if case.startswith("ncldtop") or case in ("cold", "dry", "moist"):
        variants += [ca.VARIANT_KCACHE, ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE]
    for variant in variants:
        out = run_gpu(s, 300, 64, variant=variant)
        assert bitwise_mismatches(out, ref) == {}, variant


@pytest.mark.parametrize("case", __import__("make_fixtures").EDGE_CASES)
def test_bitwise_input_edges(lib, ds, oracle_mod, case):
    """States beyond the shipped data's ranges (make_fixtures.edge_case; the oracle
    is pinned to the reference kernel on them in tests/test_oracle.py): every
    variant bit-identical to the oracle in fp64, and the exact-libm fp32 KSEG
    kernel to the fp32 restatement."""
    import make_fixtures as mf
    s = mf.edge_case(ds, case)
    ref = oracle_outputs(oracle_mod, s, 300, 64)
    for variant in (ca.VARIANT_KSEG, ca.VARIANT_KCACHE, ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE):
        out = run_gpu(s, 300, 64, variant=variant)
        assert bitwise_mismatches(out, ref) == {}, variant
    out = run_gpu(s, 300, 64, precision=ca.FP32, variant=ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM)
    ref = oracle_outputs(oracle_mod, s, 300, 64, precision=ca.FP32)
    for _, k in ca.VALIDATED:
        a = np.ascontiguousarray(out[k], dtype=np.float32).view(np.uint32)
        r = np.ascontiguousarray(ref[k], dtype=np.float32).view(np.uint32)
        assert np.array_equal(a, r), (k, int(np.count_nonzero(a != r)))


@pytest.mark.parametrize("case", __import__("make_fixtures").PARAM_CASES)
def test_bitwise_parameter_edges(lib, ds, oracle_mod, case):
    """Other time steps and the YRECLDP tuning parameters jittered together
    (make_fixtures.param_case; the host-folded reciprocals of the known divisors
    change with them): KSEG and KCACHE bit-identical to the oracle in fp64, and
    the exact-libm fp32 KSEG kernel to the fp32 restatement."""
    import make_fixtures as mf
    s = mf.param_case(ds, case)
    ref = oracle_outputs(oracle_mod, s, 300, 64)
    for variant in (ca.VARIANT_KSEG, ca.VARIANT_KCACHE):
        out = run_gpu(s, 300, 64, variant=variant)
        assert bitwise_mismatches(out, ref) == {}, variant
    out = run_gpu(s, 300, 64, precision=ca.FP32, variant=ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM)
    ref = oracle_outputs(oracle_mod, s, 300, 64, precision=ca.FP32)
    for _, k in ca.VALIDATED:
        a = np.ascontiguousarray(out[k], dtype=np.float32).view(np.uint32)
        r = np.ascontiguousarray(ref[k], dtype=np.float32).view(np.uint32)
        assert np.array_equal(a, r), (k, int(np.count_nonzero(a != r)))


def test_dwarf_tolerance_vs_reference_h5(lib, ds):
    """The dwarf's own printed check (validate_mod.F90:273-290): relL1 of every
    field vs reference.h5 within 10*eps(fp64), no '!!!!' flag."""
    out = run_gpu(ds, 100, 128, variant=ca.VARIANT_KSEG)
    eps = np.finfo(np.float64).eps
    for name, k in ca.VALIDATED:
        r = ds.reference[k].astype(np.float64)
        d = np.abs(out[k] - r).sum()
        s = np.abs(r).sum()
        rel = 0.0 if d < eps else (d / s if s >= eps else d / (1.0 + s))
        assert rel <= 10 * eps, (name, rel)


# fp32 with CLOUDSC_FP32_EXACT_LIBM: the device expf/powf are the host C
# library's single-precision algorithms too (csrc/cloudsc_libm.h), so the fp32
# kernels reproduce the fp32 restatement (JPRB=sp semantics: float storage and
# constants, expf/powf) bit for bit.  (The default fp32 forms are float-internal:
# tolerance tests below.)
EXACT = ca.FP32_EXACT_LIBM


@pytest.mark.parametrize("variant", [ca.VARIANT_KCACHE, ca.VARIANT_KSEG, ca.VARIANT_SCC])
def test_bitwise_fp32_vs_oracle(lib, ds, oracle_mod, variant):
    out = run_gpu(ds, 1000, 128, precision=ca.FP32, variant=variant | EXACT)
    ref = oracle_outputs(oracle_mod, ds, 1000, 128, precision=ca.FP32)
    bad = {}
    for _, k in ca.VALIDATED:
        a = np.ascontiguousarray(out[k], dtype=np.float32).view(np.uint32)
        r = np.ascontiguousarray(ref[k], dtype=np.float32).view(np.uint32)
        n = int(np.count_nonzero(a != r))
        if n:
            bad[k] = (n, rel_l1(out[k], ref[k]))
    assert bad == {}


@pytest.mark.parametrize("case", ["W", "M", "seed1"])
def test_bitwise_fp32_scenarios(lib, ds, scenarios, oracle_mod, case):
    import make_fixtures as mf
    s = mf.perturbed(ds, 1) if case == "seed1" else scenarios[case]
    out = run_gpu(s, 300, 64, precision=ca.FP32, variant=ca.VARIANT_KCACHE | EXACT)
    ref = oracle_outputs(oracle_mod, s, 300, 64, precision=ca.FP32)
    for _, k in ca.VALIDATED:
        a = np.ascontiguousarray(out[k], dtype=np.float32).view(np.uint32)
        r = np.ascontiguousarray(ref[k], dtype=np.float32).view(np.uint32)
        assert np.array_equal(a, r), (k, int(np.count_nonzero(a != r)))


def test_bitwise_full_size_vs_oracle(lib, ds, oracle_mod):
    """BASELINE size (163840 columns, NPROMA 64) with the bench's default kernel
    (KSEG): every validated field bit-identical to the oracle run at full size."""
    out = run_gpu(ds, 163840, 64, variant=ca.VARIANT_KSEG)
    ref = oracle_outputs(oracle_mod, ds, 163840, 64)
    assert bitwise_mismatches(out, ref) == {}


@pytest.mark.parametrize("case", ["ncldtop2", "ncldtop138", "klev3", "klev274", "aerosol", "nssopt3"])
@pytest.mark.parametrize("variant", [ca.VARIANT_KSEG, ca.VARIANT_KCACHE, ca.VARIANT_SCC])
def test_bitwise_fp32_other_configurations(lib, ds, oracle_mod, case, variant):
    """fp32 against the fp32 restatement on the configurations the fp64 suite
    pins against the reference kernel (parity-unpinned beyond the restatement:
    the reference has no fp32 C kernel)."""
    import make_fixtures as mf
    if case.startswith("ncldtop"):
        s = ds.copy()
        s.params["ncldtop"] = int(case[len("ncldtop"):])
    elif case == "klev3":
        s = sliced_levels(ds, ds.klev - 3)
        s.params["ncldtop"] = 2
    elif case == "klev274":
        s = mf.refined_levels(ds, 2)
    elif case == "aerosol":
        s = mf.with_aerosols(ds)
    else:
        s = ds.copy()
        s.params["nssopt"] = 3
    out = run_gpu(s, 300, 64, precision=ca.FP32, variant=variant | EXACT)
    ref = oracle_outputs(oracle_mod, s, 300, 64, precision=ca.FP32)
    for _, k in ca.VALIDATED:
        a = np.ascontiguousarray(out[k], dtype=np.float32).view(np.uint32)
        r = np.ascontiguousarray(ref[k], dtype=np.float32).view(np.uint32)
        assert np.array_equal(a, r), (k, int(np.count_nonzero(a != r)))


# ---- fp32 default: float-internal exp/pow (SURVEY.md §8c tolerance gates) ----
# Per field vs the fp32 restatement (glibc expf/powf): relL1 <= 1e-4 on the
# reference state (BASELINE config 4's data).  The fp32 algorithm is chaotic at
# the ulp level on other states (thresholds such as zqe < zzrh*zqsliq flip):
# moving every expf/powf result of the restatement itself by a random -1/0/+1
# ulp (oracle libm_nudge) changes its outputs by up to 2e-2 relL1 on the
# reference state and 6e-4..5e-3 on the perturbed / W / M states.  There the
# gate is evidence-based: no field may move more than 2x the worst field of
# that +-1-ulp probe (4 seeds), nor more than 1e-4 where the probe moves less.
# The probe is calibrated on expf/powf only: the fast kernels also round every
# division (1 ulp, cl_divf_fast), known-divisor division (1.5 ulp) and sqrt
# (1 ulp) differently from the restatement, and those are not nudged.  That is
# the same size of perturbation at more sites, so the floor can under-state the
# fast kernels' legitimate spread; the fixed 1e-4 gate on the reference state
# and test_fp32_fast_division_range below bound the divisions directly.


def nudge_floor(oracle_mod, s, n, nproma, seeds=(1, 2, 3, 4)):
    """Worst per-field relL1 of the fp32 restatement under +-1-ulp expf/powf nudges."""
    base = oracle_outputs(oracle_mod, s, n, nproma, precision=ca.FP32)
    worst = 0.0
    for seed in seeds:
        st, _ = oracle_mod.run_oracle(s, n, nproma, ca.FP32, libm_nudge=seed)
        o = ca.state_outputs_to_template(st.arrays, n)
        worst = max(worst, max(rel_l1(o[k], base[k]) for _, k in ca.VALIDATED))
    return worst


@pytest.mark.parametrize("variant", [ca.VARIANT_KSEG, ca.VARIANT_KCACHE, ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE])
def test_fp32_fast_libm_tolerance(lib, ds, oracle_mod, variant):
    n = 1000
    out = run_gpu(ds, n, 128, precision=ca.FP32, variant=variant)
    ref = oracle_outputs(oracle_mod, ds, n, 128, precision=ca.FP32)
    gold = {k: np.take(ds.reference[k], np.arange(n) % ds.klon, axis=-1) for _, k in ca.VALIDATED}
    fp32_gates(out, ref, gold, field_report(ref, gold))


@pytest.mark.parametrize("case", ["W", "M", "seed1", "aerosol", "nssopt3"])
def test_fp32_fast_libm_tolerance_scenarios(lib, ds, scenarios, oracle_mod, case):
    import make_fixtures as mf
    if case in ("W", "M"):
        s = scenarios[case]
    elif case == "seed1":
        s = mf.perturbed(ds, 1)
    elif case == "aerosol":
        s = mf.with_aerosols(ds)
    else:
        s = ds.copy()
        s.params["nssopt"] = 3
    out = run_gpu(s, 300, 64, precision=ca.FP32, variant=ca.VARIANT_KSEG)
    ref = oracle_outputs(oracle_mod, s, 300, 64, precision=ca.FP32)
    rep = field_report(out, ref)
    lim = max(RELL1_FP32_FAST, 2.0 * nudge_floor(oracle_mod, s, 300, 64))
    worst = max(rep.items(), key=lambda kv: kv[1][0])
    print("fp32 fast libm, %s: worst relL1 %s %.2e (gate %.2e)" % (case, worst[0], worst[1][0], lim))
    bad = {k: v[0] for k, v in rep.items() if not v[0] <= lim}
    assert bad == {}, (lim, bad)


def test_fp32_exact_libm_bit_is_ignored_in_fp64(lib, ds):
    a = run_gpu(ds, 1000, 128, variant=ca.VARIANT_KSEG)
    b = run_gpu(ds, 1000, 128, variant=ca.VARIANT_KSEG | EXACT)
    assert bitwise_mismatches(a, b) == {}


def ulp_distance(a, b):
    """|a - b| in units in the last place of float32 (sign-magnitude ordering)."""
    ia = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_fp32_fast_libm_ulp(lib):
    """The float-internal expf / powf against the glibc-algorithm forms (which
    are within 1 ulp of the exact values, tools/libm_check.cc) on the device,
    over the argument ranges CLOUDSC uses (saturation exponents -40..20, the
    snow / ice exponentials, pow bases 1e-12..1e8 with the parameter exponents
    0.333 .. 1.5 and random ones): at most 2 ulp apart, most of them equal."""
    import ctypes as C
    rng = np.random.default_rng(11)
    n = 1 << 20
    x = np.concatenate([rng.uniform(-40.0, 20.0, n // 2), rng.uniform(-87.0, 87.0, n // 2)]).astype(np.float32)
    px = (10.0 ** rng.uniform(-12.0, 8.0, n)).astype(np.float32)
    py = np.concatenate([rng.choice(np.array([0.333, 0.4, 0.5777, 0.666, 1.5, 3.0, 2.47, -1.79], np.float32),
                                    n // 2), rng.uniform(-3.0, 3.0, n // 2)]).astype(np.float32)
    res = {}
    for which in range(4):
        out = np.empty(n, np.float32)
        xs = x if which % 2 == 0 else px
        ca.check(lib.cloudsc_debug_fp32_libm(0, which, xs.ctypes.data, py.ctypes.data, out.ctypes.data, n))
        res[which] = out
    d_exp = ulp_distance(res[0], res[2])
    finite = np.isfinite(res[3]) & (res[3] > 1e-37) & (res[3] < 1e37)
    d_pow = ulp_distance(res[1][finite], res[3][finite])
    print("expf fast vs glibc: max %d ulp, %.1f %% equal; powf: max %d ulp, %.1f %% equal" % (
        d_exp.max(), 100.0 * np.mean(d_exp == 0), d_pow.max(), 100.0 * np.mean(d_pow == 0)))
    assert d_exp.max() <= 2 and d_pow.max() <= 2


def test_fp32_fast_libm_special_values(lib):
    """The float-internal expf / powf have no out-of-line fallback: their
    special cases are branch-free and must still give expf's and powf's
    answers -- overflow to +inf, underflow to 0, NaN in NaN out, pow of a zero
    base 0 (y > 0) or +inf (y < 0) -- and agree with the glibc forms at the
    edges of the range."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.array([0.0, 1.0, -1.0, 88.0, 88.7, 89.0, 100.0, 1e30, inf, -87.0, -100.0, -104.0, -200.0, -inf, nan],
                 np.float32)
    px = np.array([0.0, 0.0, 1.0, 2.0, 1e-30, 1e30, inf, inf, 1e-38, nan, 2.0, 0.5], np.float32)
    py = np.array([0.5, -0.5, 3.0, 0.5, 0.666, 1.5, 0.5, -0.5, 0.4, 0.5, nan, 200.0], np.float32)
    out = {}
    for which, (a, b) in {0: (x, x), 2: (x, x), 1: (px, py), 3: (px, py)}.items():
        o = np.empty(a.size, np.float32)
        ca.check(lib.cloudsc_debug_fp32_libm(0, which, a.ctypes.data, b.ctypes.data, o.ctypes.data, a.size))
        out[which] = o
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        want_e = np.exp(x.astype(np.float64)).astype(np.float32)
        want_p = np.power(px.astype(np.float64), py.astype(np.float64)).astype(np.float32)
    for fast, ref, want in ((out[0], out[2], want_e), (out[1], out[3], want_p)):
        fin = np.isfinite(want) & (want != 0)
        # special values exactly; finite results within 2 ulp of the glibc forms
        assert np.array_equal(np.isnan(fast), np.isnan(want)), (fast, want)
        assert np.array_equal(fast[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), (fast, want)
        assert ulp_distance(fast[fin], ref[fin]).max() <= 2, (fast[fin], ref[fin])


def test_fp32_fast_division_range(lib):
    """The fast kernels' division (cl_divf_fast: v_rcp_f32 + one residual
    correction, no div_scale / div_fixup) against IEEE float division, over its
    documented range (cloudsc_dev.h): normal divisors 2^-126 <= |d| < 2^126
    with finite normal quotients are within 1 ulp and 0/d is 0; the exact
    kernels' division (cl_div) is the IEEE quotient everywhere in that range.
    Outside it (|d| below 2^-126 where the reciprocal overflows, zero divisors)
    the fast form is not IEEE; the test records that behaviour so a change shows."""
    rng = np.random.default_rng(5)
    n = 1 << 20
    d = (np.sign(rng.uniform(-1, 1, n)) * 2.0 ** rng.uniform(-125.9, 125.9, n)).astype(np.float32)
    num = (np.sign(rng.uniform(-1, 1, n)) * 2.0 ** rng.uniform(-60.0, 60.0, n)).astype(np.float32)
    num[:1000] = 0.0
    # CLOUDSC-like operands: ratios of physical quantities near 1e-12 .. 1e5
    d[1000:200000] = (10.0 ** rng.uniform(-12.0, 5.0, 199000)).astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        want = (num / d).astype(np.float32)
    ok = np.isfinite(want) & ((want == 0) | (np.abs(want) >= np.finfo(np.float32).tiny))
    out = {}
    for which in (4, 5):
        o = np.empty(n, np.float32)
        ca.check(lib.cloudsc_debug_fp32_libm(0, which, num.ctypes.data, d.ctypes.data, o.ctypes.data, n))
        out[which] = o
    assert np.all(out[4][:1000] == 0.0)
    dist = ulp_distance(out[4][ok], want[ok])
    print("fast fp32 division: max %d ulp, %.2f %% IEEE" % (dist.max(), 100.0 * np.mean(dist == 0)))
    assert dist.max() <= 1
    mid = ok & (np.abs(want) >= 2.0 ** -100) & (np.abs(want) <= 2.0 ** 100)   # no residual underflow
    assert np.array_equal(out[5][mid].view(np.int32), want[mid].view(np.int32))
    # out of range: tiny / zero divisors (documented: not the IEEE answer)
    tn = np.array([0.0, 1.0, 1e-30, 0.0, 1.0], np.float32)
    td = np.array([1e-40, 1e-40, 1e-39, 0.0, 0.0], np.float32)
    o = np.empty(tn.size, np.float32)
    ca.check(lib.cloudsc_debug_fp32_libm(0, 4, tn.ctypes.data, td.ctypes.data, o.ctypes.data, tn.size))
    print("fast fp32 division out of range:", list(zip(tn, td, o)))
    assert not np.isfinite(o[0]) and not np.isfinite(o[3]), o
