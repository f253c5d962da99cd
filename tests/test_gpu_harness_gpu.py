"""Positive control of the comparisons in tests/gpu_harness.py, without a physics launch: two field sets with
the same bytes but one flipped bit."""
import pytest

import cloudsc_amd as ca
from gpu_harness import DeviceProblem, NAMES, PATTERN, differing, host_inputs, raw_bits
from gpu_harness import lib, hip, restore_knobs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def test_one_flipped_bit_is_found_on_the_device_and_on_the_host(lib, hip, ds):
    p = DeviceProblem(lib, hip, ds, 70, 32, ca.FP64)
    try:
        a, b = p.device_fields(), p.device_fields()
        host = host_inputs(ds, 70, 32, ca.FP64, PATTERN)
        a.upload(host)
        b.upload(host)

        def found():
            on_host = differing({k: a.download_raw(k) for k in NAMES}, {k: b.download_raw(k) for k in NAMES}, NAMES)
            return p.mismatches(a.f, b.f, NAMES), on_host
        assert found() == ({}, [])
        flipped = host["pfplsn"].copy()
        raw_bits(flipped).reshape(flipped.shape + (8,))[1, 5, 3, 0] ^= 1      # column 35, level 5: the lowest bit
        a.upload({"pfplsn": flipped})
        assert found() == ({"pfplsn": 1}, ["pfplsn"])
        a.upload({"pfplsn": host["pfplsn"]})
        assert found() == ({}, [])
    finally:
        p.close()
