"""Narrow NPROMA blocks packed into full waves, on the device.  Packing changes
no lane's arithmetic, so every comparison is on raw bits: against the fp64
oracle, the mixed-precision contract (tests/mixed_expected.py), the fp32
restatement, and the unpacked kernels on the same buffers."""
import numpy as np
import pytest

import cloudsc_amd as ca
import mixed_expected as mx
from gpu_harness import NAMES, Run, oracle_columns, pattern_like, widened_bits as bits
from gpu_harness import lib, restore_knobs  # noqa: F401  (fixtures)
from host_harness import configured

pytestmark = pytest.mark.gpu

# (ngptot, nproma): pack | what it exercises
SHAPES = [
    (100, 32),   # 2  | last block holds 4 columns
    (100, 16),   # 4  | last group holds 3 blocks
    (100, 8),    # 8  | last group holds 5 blocks
    (70, 1),     # 64 | last group holds 6 blocks
    (100, 24),   # 2  | 48 lanes
    (100, 5),    # 12 | 60 lanes
    (100, 33),   # 1  | must be untouched
]
PACK_OF = {32: 2, 16: 4, 8: 8, 1: 64, 24: 2, 5: 12, 33: 1}
KCACHES = [ca.VARIANT_KCACHE, ca.VARIANT_KSEG]


def differing(out, ref):
    return {k: int(np.count_nonzero(bits(out[k]) != bits(ref[k]))) for k in NAMES
            if not np.array_equal(bits(out[k]), bits(ref[k]))}


def geometry_pack(ds, precision, variant, ngptot, nproma):
    return ca.launch_geometry(precision, variant & 0xff, ngptot, nproma, ds.klev)["pack"]


# ---------------------------------------------------------------------------
# fp64 against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ngptot,nproma", SHAPES)
def test_fp64_packed_vs_oracle_device_fields(lib, ds, oracle_mod, ngptot, nproma):
    ref = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma)
    r = Run(lib, ds, ngptot, nproma)
    try:
        for variant in KCACHES:
            out = r.columns(r.launch(variant, 1))
            assert geometry_pack(ds, ca.FP64, variant, ngptot, nproma) == PACK_OF[nproma]
            assert differing(out, ref) == {}, variant
    finally:
        r.close()


@pytest.mark.parametrize("ngptot,nproma", SHAPES)
def test_fp64_packed_vs_oracle_state(lib, ds, oracle_mod, ngptot, nproma):
    """Through GpuState: repeated steps continue the workspace's counters and flag stamps."""
    ref = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma)
    ca.narrow_pack(1)
    g = ca.GpuState(ds, ngptot, nproma, ca.FP64)
    try:
        g.run(ca.VARIANT_KSEG, 1)
        kseg = g.outputs()
        g.run(ca.VARIANT_KSEG, 3)
        kseg3 = g.outputs()
        ca.narrow_pack(0)                      # the same workspace, unpacked, and packed again
        g.run(ca.VARIANT_KSEG, 1)
        off = g.outputs()
        ca.narrow_pack(1)
        g.run(ca.VARIANT_KSEG, 1)
        again = g.outputs()
        g.run(ca.VARIANT_KCACHE, 1)
        kcache = g.outputs()
    finally:
        g.close()
    for out in (kseg, kseg3, off, again, kcache):
        assert differing(out, ref) == {}


# ---------------------------------------------------------------------------
# mixed against the contract, fp32 against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ngptot,nproma", [(100, 32), (100, 8)])
def test_mixed_packed_vs_contract(lib, ds, oracle_mod, ngptot, nproma):
    exp = mx.expected(oracle_mod, ds, ngptot, nproma, key="ref100")
    r = Run(lib, ds, ngptot, nproma, ca.MIXED)
    try:
        ca.narrow_pack(1)
        for variant in KCACHES:
            assert geometry_pack(ds, ca.MIXED, variant, ngptot, nproma) == PACK_OF[nproma]
            assert mx.mismatches(r.columns(r.launch(variant, 1)), exp) == {}, variant
    finally:
        r.close()


def test_fp32_exact_libm_packed_vs_restatement(lib, ds, oracle_mod):
    ngptot, nproma = 100, 16
    ref = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma, ca.FP32)
    r = Run(lib, ds, ngptot, nproma, ca.FP32)
    try:
        for variant in KCACHES:
            out = r.columns(r.launch(variant | ca.FP32_EXACT_LIBM, 1))
            assert differing(out, ref) == {}, variant
    finally:
        r.close()


# ---------------------------------------------------------------------------
# packed against unpacked on the same buffers; padding
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [ca.FP64, ca.FP32, ca.MIXED])
@pytest.mark.parametrize("ngptot,nproma", SHAPES)
def test_packed_equals_unpacked_and_padding_untouched(lib, ds, ngptot, nproma, precision):
    """The default kernels of every precision (fp32: the float-internal exp/pow),
    on buffers one block longer than the run: packed == unpacked over the whole
    buffers, and the lanes jl >= bsize of the last block and everything past the
    last block still hold the byte pattern."""
    r = Run(lib, ds, ngptot, nproma, precision, extra_blocks=1)
    try:
        nb, tail = r.nb, ngptot - (r.nb - 1) * nproma
        for variant in KCACHES:
            off = r.launch(variant, 0)
            on = r.launch(variant, 1)
            for k in NAMES:
                assert np.array_equal(bits(on[k]), bits(off[k])), (variant, k)
                a, pat = on[k], pattern_like(r.host[k]).astype(np.float64)
                assert a.shape[0] == nb + 1
                assert np.array_equal(bits(a[nb:]), bits(pat[nb:])), (variant, k, "past the last block")
                assert np.array_equal(bits(a[nb - 1, ..., tail:]), bits(pat[nb - 1, ..., tail:])), (variant, k, "padding")
                assert not np.array_equal(bits(a[:nb - 1]), bits(pat[:nb - 1])) or nb == 1, (variant, k, "not written")
                assert np.all(np.isfinite(a[nb - 1, ..., :tail])), (variant, k)
    finally:
        r.close()


# ---------------------------------------------------------------------------
# KSEG hand-offs across packed groups
# ---------------------------------------------------------------------------
KSEG_SCHEDULES = ((1, 1), (1, 3), (2, 1), (2, 3), (3, 1), (3, 3))


@pytest.mark.parametrize("ngptot,nproma", [(100, 16), (70, 1)])
def test_kseg_handoffs_across_packed_groups(lib, ds, oracle_mod, ngptot, nproma):
    ref = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma)
    r = Run(lib, ds, ngptot, nproma)
    try:
        for sched in KSEG_SCHEDULES:
            out = r.columns(r.launch(ca.VARIANT_KSEG, 1, sched))
            g = ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, ngptot, nproma, ds.klev)
            assert g["workgroups"] == min(sched[1], sched[0] * g["units"]), sched
            assert differing(out, ref) == {}, sched
    finally:
        r.close()


# ---------------------------------------------------------------------------
# aerosols, host pipeline, restore
# ---------------------------------------------------------------------------
def test_aerosol_kernels_packed(lib, ds, oracle_mod):
    s = configured(ds, "aerosol")
    assert s.params["laericesed"] and s.params["laericeauto"]
    ngptot, nproma = 100, 16
    ref = oracle_columns(oracle_mod, s, "aerosol", ngptot, nproma)
    r = Run(lib, s, ngptot, nproma)
    try:
        ca.narrow_pack(1)
        for variant in KCACHES:
            assert ca.launch_geometry(ca.FP64, variant, ngptot, nproma, s.klev, laer=True)["pack"] == 4
            assert differing(r.columns(r.launch(variant, 1)), ref) == {}, variant
    finally:
        r.close()
    assert differing(ref, oracle_columns(oracle_mod, ds, "ds", ngptot, nproma)) != {}    # the aerosol inputs matter


def test_host_pipeline_packed_equals_unpacked(lib, ds, oracle_mod):
    ngptot, nproma = 130, 32
    ref = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma)
    hp = ca.HostPipeline(ds, ngptot, nproma, chunk_blocks=2, nstreams=2)
    try:
        outs = {}
        for pack in (0, 1):
            ca.narrow_pack(pack)
            hp.run(ca.VARIANT_KSEG)
            outs[pack] = {k: np.array(v) for k, v in hp.outputs().items()}
    finally:
        hp.close()
    assert differing(outs[1], outs[0]) == {}
    assert differing(outs[1], ref) == {}


def test_restore_default_then_wide_blocks(lib, ds, oracle_mod):
    """The closing case: the default mode again, and NPROMA 64 as before."""
    ca.narrow_pack(-1)
    ngptot, nproma = 130, 64
    assert ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, ngptot, nproma, ds.klev)["pack"] == 1
    ref = oracle_columns(oracle_mod, ds, "ds", ngptot, nproma)
    r = Run(lib, ds, ngptot, nproma)
    try:
        for variant in KCACHES:
            assert differing(r.columns(r.launch(variant, -1)), ref) == {}, variant
    finally:
        r.close()
