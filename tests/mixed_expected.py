"""TEST INFRASTRUCTURE ONLY -- the expected value of a CLOUDSC_MIXED run.

The contract of include/cloudsc_amd.h, bit for bit over the 20 output fields
and plude:

    expected = float32( oracle_fp64( float64( float32(inputs) ) ) )

with oracle_fp64 the unchanged fp64 restatement (oracle/) or, where it is
built, the reference kernel itself (oracle/_ref).  Nothing here calls the
library under test."""
import numpy as np

import cloudsc_amd as ca

SUBNORMAL_BELOW = float(np.finfo(np.float32).tiny)   # 2^-126


def rounded_inputs(ds):
    """Copy of ds whose real inputs (plude included) are float32 values held in
    float64: numpy.astype(float32) rounds to nearest even, the widening is exact."""
    s = ds.copy()
    for k, a in ds.inputs.items():
        if k != "ktype":
            with np.errstate(over="ignore", under="ignore"):
                s.inputs[k] = np.ascontiguousarray(a.astype(np.float32).astype(np.float64))
    return s


_cache = {}


def expected(oracle_mod, ds, ngptot, nproma, key=None, runner="oracle"):
    """{field: float32 array [..][ngptot]} for the 21 validated fields.  key: a
    name for ds under which the result is kept for the other tests (None: not kept)."""
    ck = (key, ngptot, nproma, runner)
    if key is not None and ck in _cache:
        return _cache[ck]
    s = rounded_inputs(ds)
    if runner == "ref":
        st, _ = oracle_mod.run_ref(s, ngptot, nproma)
    else:
        st, _ = oracle_mod.run_oracle(s, ngptot, nproma, ca.FP64)
    with np.errstate(over="ignore", under="ignore"):
        out = {k: np.ascontiguousarray(ca.blocks_to_columns(st.arrays[k], ngptot).astype(np.float32))
               for _, k in ca.VALIDATED}
    for a in out.values():
        a.setflags(write=False)
    if key is not None:
        _cache[ck] = out
    return out


def as_f32(a):
    """A downloaded field (float32, or float64 holding float32 values) as float32."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a
    b = a.astype(np.float32)
    assert np.array_equal(b.astype(np.float64), a, equal_nan=True), "not float32 values"
    return b


def mismatches(out, exp):
    """{field: differing elements} on raw bits (view(uint32)) over the 21 fields."""
    bad = {}
    for _, k in ca.VALIDATED:
        a = as_f32(out[k]).view(np.uint32)
        e = np.ascontiguousarray(exp[k]).view(np.uint32)
        assert a.shape == e.shape, (k, a.shape, e.shape)
        n = int(np.count_nonzero(a != e))
        if n:
            bad[k] = n
    return bad


def all_finite(exp):
    return all(bool(np.all(np.isfinite(a))) for a in exp.values())


def subnormal_count(exp):
    """Compared output elements that are non-zero float32 subnormals."""
    return sum(int(np.count_nonzero((a != 0) & (np.abs(a) < SUBNORMAL_BELOW))) for a in exp.values())


def rel_l1(out, gold):
    """Per-field relative L1 error as ERROR_PRINT takes it (sum|d| / sum|ref|)."""
    rep = {}
    for _, k in ca.VALIDATED:
        _, _, _, errsum, refsum = ca.field_stats(out[k], gold[k])
        rep[k] = ca.rel_error(errsum, refsum)[0]
    return rep
