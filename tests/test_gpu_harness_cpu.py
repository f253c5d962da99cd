"""Positive controls of tests/gpu_harness.py that need no GPU: host_inputs fills what it says and nothing
else, raw_bits tells apart what == does not, and columns drops exactly the padding lanes."""
import numpy as np
import pytest

import cloudsc_amd as ca
from gpu_harness import columns, host_inputs, raw_bits

PATTERN = 0xC3


@pytest.mark.parametrize("precision", [ca.FP64, ca.MIXED], ids=["fp64", "mixed"])
@pytest.mark.parametrize("ngptot,nproma", [(70, 32), (64, 64)])        # a partial last block, and none
def test_host_inputs_fills_the_outputs_and_plude_padding_only(ds, ngptot, nproma, precision):
    ref = ca.make_host_state(ds, ngptot, nproma, precision).arrays
    got = host_inputs(ds, ngptot, nproma, precision, PATTERN)
    assert sorted(got) == sorted(ref) and "plude" in got and set(ca.OUTPUT_FIELDS) <= set(got)
    nb = ca.nblocks_of(ngptot, nproma)
    for name, a in got.items():
        assert a.dtype == ref[name].dtype and a.shape == ref[name].shape, name
        each = raw_bits(a).reshape(a.shape + (a.itemsize,))             # the bytes of every element
        if name in ca.OUTPUT_FIELDS:
            assert (each == PATTERN).all(), name
        elif name == "plude":
            pad = np.zeros(a.shape, dtype=bool)
            pad[nb - 1, ..., ngptot - (nb - 1) * nproma:] = True
            assert int(pad.sum()) == (0 if ngptot % nproma == 0 else a.shape[1] * (nb * nproma - ngptot))
            assert (each[pad] == PATTERN).all()
            assert not (each[~pad] == PATTERN).all(axis=-1).any()      # and nowhere else
            assert np.array_equal(each[~pad], raw_bits(ref[name]).reshape(each.shape)[~pad])
        else:
            assert np.array_equal(each, raw_bits(ref[name]).reshape(each.shape)), name


def test_raw_bits_tells_zero_signs_and_nan_payloads_apart():
    zeros = np.array([0.0]), np.array([-0.0])
    assert np.array_equal(*zeros) and not np.array_equal(raw_bits(zeros[0]), raw_bits(zeros[1]))
    nans = np.array([0x7FF8000000000001, 0x7FF8000000000002], dtype=np.uint64).view(np.float64)
    assert np.isnan(nans).all() and not np.array_equal(raw_bits(nans[:1]), raw_bits(nans[1:]))
    assert np.array_equal(raw_bits(nans), raw_bits(nans.copy()))


@pytest.mark.parametrize("ngptot,nproma", [(70, 32), (64, 64)])
def test_columns_drops_exactly_the_padding_lanes(ngptot, nproma):
    nb, rows = ca.nblocks_of(ngptot, nproma), 3
    g = np.arange(nb * nproma).reshape(nb, 1, nproma) + 1000 * np.arange(rows).reshape(1, rows, 1)
    blocks = np.where(g % 1000 < ngptot, g, -1).astype(np.float64)       # -1 in the lanes past the last column
    got = columns(blocks, ngptot)
    assert got.shape == (rows, ngptot) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, np.arange(ngptot)[None, :] + 1000 * np.arange(rows)[:, None])
