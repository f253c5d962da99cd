"""CLOUDSC_MIXED without a GPU: cloudsc_cpu_run_precision compiles the phase
functions the kernels are built from for the host with float storage, so the
storage / compute split (widening load, narrowing store, lane offsets by the
storage size) is pinned bit for bit against

    expected = float32( oracle_fp64( float64( float32(inputs) ) ) )

(tests/mixed_expected.py), on raw bits over the 20 outputs and plude."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca
import mixed_expected as mx
from host_harness import configured


def cpu_mixed(ds, ngptot, nproma, nthreads=4):
    st, _ = ca.cpu_run(ds, ngptot, nproma, nthreads=nthreads, precision=ca.MIXED)
    for _, k in ca.VALIDATED:
        assert st.arrays[k].dtype == np.float32
    return ca.state_outputs_to_template(st.arrays, ngptot)


# one partial last block | one block | three blocks, partial tail | fewer lanes than NPROMA
SHAPES = [(100, 32), (100, 100), (130, 64), (7, 16)]


@pytest.mark.parametrize("ngptot,nproma", SHAPES)
def test_cpu_mixed_bitwise_shapes(ds, oracle_mod, ngptot, nproma):
    exp = mx.expected(oracle_mod, ds, ngptot, nproma, key="ref100")
    assert mx.all_finite(exp)
    assert mx.mismatches(cpu_mixed(ds, ngptot, nproma), exp) == {}


CONFIGS = ["nssopt0", "nssopt2", "nssopt3", "aerosol", "aerosol_sed", "aerosol_auto", "ncldtop2", "ncldtop138",
           "klev3", "klev16", "cold", "dry", "moist", "seed1", "seed2"]


@pytest.mark.parametrize("case", CONFIGS)
def test_cpu_mixed_bitwise_configurations(ds, oracle_mod, case):
    s = configured(ds, case)
    assert s.klev + 1 == 138 or not case == "ncldtop138"
    exp = mx.expected(oracle_mod, s, 130, 64, key=case)
    assert mx.mismatches(cpu_mixed(s, 130, 64), exp) == {}


def test_cpu_mixed_thread_invariance(ds, oracle_mod):
    exp = mx.expected(oracle_mod, ds, 130, 64, key="ref100")
    for nthreads in (1, 4):
        assert mx.mismatches(cpu_mixed(ds, 130, 64, nthreads=nthreads), exp) == {}, nthreads


def test_cpu_mixed_vs_reference_kernel(ds, oracle_mod):
    """The same identity with the reference kernel itself in place of the restatement."""
    if not oracle_mod.ref_available():
        pytest.skip("oracle/_ref not built (no reference checkout)")
    exp = mx.expected(oracle_mod, ds, 100, 32, key="ref100", runner="ref")
    assert mx.mismatches(cpu_mixed(ds, 100, 32), exp) == {}


F32_SENTINEL = np.uint32(0x7FA5A5A5)   # a NaN with a payload no arithmetic produces
I32_SENTINEL = np.int32(0x5A5A5A5A)


def test_cpu_mixed_inactive_lanes_untouched(ds, oracle_mod):
    """Lanes beyond NGPTOT in the last block: neither read (the active lanes do
    not change) nor written (the sentinel is still there)."""
    ngptot, nproma = 100, 32
    bsize = ngptot - (ca.nblocks_of(ngptot, nproma) - 1) * nproma
    st = ca.make_host_state(ds, ngptot, nproma, ca.MIXED)
    for k, a in st.arrays.items():
        if a.dtype == np.float32:
            a.view(np.uint32)[-1, ..., bsize:] = F32_SENTINEL
        else:
            a[-1, ..., bsize:] = I32_SENTINEL
    before = {k: a.copy() for k, a in st.arrays.items()}
    ca.cpu_run_state(ds, st, nthreads=2)
    outs = [k for _, k in ca.VALIDATED]
    for k, a in st.arrays.items():
        if a.dtype == np.float32:
            assert np.all(a.view(np.uint32)[-1, ..., bsize:] == F32_SENTINEL), k
        else:
            assert np.all(a[-1, ..., bsize:] == I32_SENTINEL), k
        if k not in outs:
            assert np.array_equal(a.view(np.uint32), before[k].view(np.uint32)), k
    exp = mx.expected(oracle_mod, ds, ngptot, nproma, key="ref100")
    assert mx.mismatches(ca.state_outputs_to_template(st.arrays, ngptot), exp) == {}


def test_cpu_run_precision_codes(ds, oracle_mod):
    """FP64 through the new entry point is cloudsc_cpu_run; FP32 and unknown codes are refused."""
    lib = ca.gpu_lib()
    p = ca.Params.from_dict(ds.params)
    st = ca.make_host_state(ds, 64, 32, ca.FP32)
    f = st.fields()
    assert lib.cloudsc_cpu_run_precision(1, ca.FP32, 64, 32, ds.klev, C.byref(p), C.byref(f), None) == ca.EINVAL
    for code in (0, 2, 16):
        assert lib.cloudsc_cpu_run_precision(1, code, 64, 32, ds.klev, C.byref(p), C.byref(f), None) == ca.EINVAL
    assert lib.cloudsc_cpu_run_precision(1, ca.MIXED, 0, 32, ds.klev, C.byref(p), C.byref(f), None) == ca.EINVAL
    st64, _ = ca.cpu_run(ds, 100, 32, nthreads=2, precision=ca.FP64)
    ref, _ = oracle_mod.run_oracle(ds, 100, 32)
    for _, k in ca.VALIDATED:
        a = ca.blocks_to_columns(st64.arrays[k], 100)
        r = ca.blocks_to_columns(ref.arrays[k], 100)
        assert np.array_equal(a.view(np.uint64), r.view(np.uint64)), k


def test_precision_codes_and_sizes(ds):
    """The codes keep their values, mixed has one of its own; the KSEG
    workspace of mixed is fp64's (the carried state stays double); SCC has no
    mixed form; the public structs are unchanged."""
    lib = ca.gpu_lib()
    assert (ca.FP64, ca.FP32) == (8, 4) and ca.MIXED not in (4, 8)
    for ngptot, nproma in [(130, 16), (300, 128), (163840, 64)]:
        a = lib.cloudsc_gpu_scratch_bytes(ca.MIXED, ca.VARIANT_KSEG, ngptot, nproma, ds.klev)
        assert a > 0 and a == lib.cloudsc_gpu_scratch_bytes(ca.FP64, ca.VARIANT_KSEG, ngptot, nproma, ds.klev)
        assert a > lib.cloudsc_gpu_scratch_bytes(ca.FP32, ca.VARIANT_KSEG, ngptot, nproma, ds.klev)
    assert lib.cloudsc_gpu_scratch_bytes(ca.MIXED, ca.VARIANT_KCACHE, 130, 64, ds.klev) == 0
    assert lib.cloudsc_gpu_scratch_bytes(ca.MIXED, ca.VARIANT_SCC, 130, 64, ds.klev) == -1
    assert lib.cloudsc_gpu_scratch_bytes(5, ca.VARIANT_KSEG, 130, 64, ds.klev) == -1
    # 133 doubles + 18 ints, 48 pointers, 2 ints + 28 pointers, 2 ints + 21 pointers, 7 doubles
    assert [lib.cloudsc_abi_sizeof(i) for i in range(5)] == [1136, 384, 232, 176, 56]
    assert [lib.cloudsc_abi_sizeof(i) for i in range(5)] == [C.sizeof(ca.Params), C.sizeof(ca.Fields),
                                                            C.sizeof(ca.Template), C.sizeof(ca.Reference),
                                                            C.sizeof(ca.Stats)]


def test_dwarf_cli_mixed_cpu():
    """`dwarf-cloudsc-amd 2 1000 64 --precision mixed --variant cpu`: the table,
    reported the way fp32's is (no gate without --tol, exit status 0)."""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(ca.LIB_PATH), "dwarf-cloudsc-amd")
    r = subprocess.run([exe, "2", "1000", "64", "--precision", "mixed", "--variant", "cpu"], capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-1000:])
    assert r.returncode == 0
    assert "CLOUDSC-AMD: mixed, variant cpu" in r.stdout
    assert "VALIDATION: reported only (mixed vs the fp64 reference" in r.stdout
    rows = [l for l in r.stdout.splitlines() if re.match(r"\s+\S+ \dD\d ", l)]
    assert len(rows) == 21
