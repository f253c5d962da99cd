"""Narrow NPROMA blocks packed into full waves, without a GPU: the launch
geometry the library reports (cloudsc_gpu_launch_geometry is host arithmetic),
the knob that overrides the default, and the workspace size, which packing
must not change."""
import pytest

import cloudsc_amd as ca

NGPTOT = 100
NPROMAS = [1, 5, 8, 16, 24, 32, 33, 64, 128]
PACK = [64, 12, 8, 4, 2, 2, 1, 1, 1]
LANES = [64, 60, 64, 64, 48, 64, 33, 64, 64]
KCACHES = [ca.VARIANT_KCACHE, ca.VARIANT_KSEG]
PRECISIONS = [ca.FP64, ca.FP32, ca.MIXED]


def ceil_div(a, b):
    return -(-a // b)


@pytest.fixture
def pack_mode():
    """Sets the process-wide mode for a test and puts the default back."""
    ca.gpu_lib()
    yield ca.narrow_pack
    ca.narrow_pack(-1)
    ca.kseg_schedule(0, 0)


@pytest.mark.parametrize("variant", KCACHES)
def test_geometry_packed(ds, pack_mode, variant):
    pack_mode(1)
    for nproma, pack, lanes in zip(NPROMAS, PACK, LANES):
        g = ca.launch_geometry(ca.FP64, variant, NGPTOT, nproma, ds.klev)
        nblocks, nsub = ceil_div(NGPTOT, nproma), ceil_div(nproma, 64)
        assert (g["pack"], g["lanes"]) == (pack, lanes), nproma
        assert g["units"] == ceil_div(nblocks, pack) * nsub, nproma
        if variant == ca.VARIANT_KCACHE:
            # one workgroup per group of blocks; packed workgroups are one full wave
            assert g["workgroups"] == ceil_div(nblocks, pack), nproma
            assert g["wg_threads"] == (64 if pack > 1 else nproma), nproma
        else:
            # two level segments by default; never more workgroups than items
            assert 1 <= g["workgroups"] <= 2 * g["units"], nproma
            assert g["wg_threads"] == (64 if pack > 1 else min(nproma, 64)), nproma


@pytest.mark.parametrize("variant", KCACHES)
def test_geometry_unpacked(ds, pack_mode, variant):
    pack_mode(0)
    for nproma in NPROMAS:
        g = ca.launch_geometry(ca.FP64, variant, NGPTOT, nproma, ds.klev)
        nblocks, nsub = ceil_div(NGPTOT, nproma), ceil_div(nproma, 64)
        assert g["pack"] == 1
        assert g["lanes"] == min(nproma, 64)
        assert g["units"] == nblocks * nsub
        if variant == ca.VARIANT_KCACHE:
            assert (g["workgroups"], g["wg_threads"]) == (nblocks, nproma)
        else:
            assert g["wg_threads"] == min(nproma, 64)
            assert 1 <= g["workgroups"] <= 2 * nblocks * nsub


def test_kseg_grid_follows_schedule_override(ds, pack_mode):
    """cloudsc_debug_set_kseg_schedule acts on groups: the grid is the requested
    one, capped at segments x groups."""
    pack_mode(1)
    ca.kseg_schedule(3, 3)
    g = ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, 100, 16, ds.klev)
    assert (g["pack"], g["units"], g["workgroups"]) == (4, 2, 3)
    ca.kseg_schedule(1, 3)
    g = ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, 100, 16, ds.klev)
    assert (g["units"], g["workgroups"]) == (2, 2)


def test_scratch_bytes_do_not_depend_on_packing(ds, pack_mode):
    lib = ca.gpu_lib()
    sizes = {}
    for mode in (0, 1, -1):
        pack_mode(mode)
        sizes[mode] = [lib.cloudsc_gpu_scratch_bytes(p, v, NGPTOT, n, ds.klev)
                       for p in PRECISIONS for v in KCACHES for n in NPROMAS]
    assert sizes[0] == sizes[1] == sizes[-1]
    assert all(s >= 0 for s in sizes[0])
    # the carried state keeps [nblocks][19][nproma] values of the compute type after the control words
    pack_mode(1)
    b = lib.cloudsc_gpu_scratch_bytes(ca.FP64, ca.VARIANT_KSEG, 100, 16, ds.klev)
    assert b == 1536 + 7 * 19 * 16 * 8


def test_every_precision_and_aerosol_configuration_packs(ds, pack_mode):
    """No configuration had to stay unpacked for registers (all 16 packed kernels
    compile without spills, profiles/narrow_pack/kernel_resources.txt): the
    geometry is the same with and without the aerosol kernels, in every precision."""
    pack_mode(1)
    for precision in PRECISIONS:
        for variant in KCACHES:
            for laer in (False, True):
                for nproma, pack in zip(NPROMAS, PACK):
                    g = ca.launch_geometry(precision, variant, NGPTOT, nproma, ds.klev, laer=laer)
                    assert g["pack"] == pack, (precision, variant, laer, nproma)
    exact = ca.launch_geometry(ca.FP32, ca.VARIANT_KSEG | ca.FP32_EXACT_LIBM, NGPTOT, 16, ds.klev)
    assert exact["pack"] == 4


def test_scc_variants_never_pack(ds, pack_mode):
    pack_mode(1)
    for variant in (ca.VARIANT_SCC, ca.VARIANT_SCC_PRIVATE):
        for nproma in NPROMAS:
            g = ca.launch_geometry(ca.FP64, variant, NGPTOT, nproma, ds.klev)
            nblocks = ceil_div(NGPTOT, nproma)
            assert g["pack"] == 1
            assert g["lanes"] == min(nproma, 64)
            assert (g["workgroups"], g["wg_threads"]) == (nblocks, nproma)


def test_lane_offsets_must_fit_32_bits(pack_mode):
    """pack * 5 * (klev + 1) * nproma * 8 bytes: beyond 2^32 the launch stays unpacked."""
    pack_mode(1)
    assert ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, 100, 32, 1677720)["pack"] == 2   # 2560 * 1677721 < 2^32
    assert ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, 100, 32, 1677721)["pack"] == 1
    assert ca.launch_geometry(ca.FP64, ca.VARIANT_KCACHE, 100, 1, 2000000)["pack"] == 1


def test_bad_arguments(ds, pack_mode):
    pack_mode(1)
    bad = [
        (ca.FP64, ca.VARIANT_KSEG, 0, 16, ds.klev),
        (ca.FP64, ca.VARIANT_KSEG, 100, 0, ds.klev),
        (ca.FP64, ca.VARIANT_KSEG, 100, -4, ds.klev),
        (ca.FP64, ca.VARIANT_KSEG, 100, 16, 1),
        (ca.FP64, ca.VARIANT_KCACHE, 100, 257, ds.klev),      # KCACHE: one workgroup per block
        (ca.FP64, ca.VARIANT_KSEG, 100, (1 << 24) + 1, ds.klev),
        (3, ca.VARIANT_KSEG, 100, 16, ds.klev),               # no such precision
        (ca.FP64, 99, 100, 16, ds.klev),                      # no such variant
        (ca.FP64, ca.VARIANT_KSEG | 0x1000, 100, 16, ds.klev),
        (ca.MIXED, ca.VARIANT_SCC, 100, 16, ds.klev),         # mixed: the k-caching kernels only
    ]
    for args in bad:
        with pytest.raises(ca.CloudscError) as e:
            ca.launch_geometry(*args)
        assert e.value.code == ca.EINVAL, args
    assert ca.gpu_lib().cloudsc_gpu_launch_geometry(ca.FP64, ca.VARIANT_KSEG, 100, 16, ds.klev, 0, None) == ca.EINVAL
    assert ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, 100, 1 << 24, ds.klev)["pack"] == 1


def test_default_mode_is_one_of_the_two(ds, pack_mode):
    """Negative = the measured default: per width, either the packed or the
    unpacked geometry, nothing else."""
    for nproma in NPROMAS:
        pack_mode(-1)
        d = ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, NGPTOT, nproma, ds.klev)
        pack_mode(0)
        off = ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, NGPTOT, nproma, ds.klev)
        pack_mode(1)
        on = ca.launch_geometry(ca.FP64, ca.VARIANT_KSEG, NGPTOT, nproma, ds.klev)
        assert d in (off, on), nproma
