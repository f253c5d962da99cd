"""TEST INFRASTRUCTURE ONLY -- what the tests of the advancing step (cloudsc_*_run_advance, cloudsc_*_fields_advance)
share: the member names, the states and shapes, and the expectation, which never comes from the code under test.
The one definition, for X in {t, q, a, cld[0..3]}:

    X0    = fl(X  + fl(ptsphy * tendency_tmp))
    X_new = fl(X0 + fl(ptsphy * loc))

each operation a NumPy ufunc call of its own (nothing fuses) in the working type.  fp64: loc is the oracle's.
Mixed: float32 of the fp64 expectation on float64(float32 inputs).  fp32: the two lines in float32 on an fp32 loc
that the caller supplies (the ordinary fp32 step's, existing code).  Nothing here calls the library under test."""
import numpy as np

import cloudsc_amd as ca
import form_state_cases as fs
import mixed_expected as mx

STATE = ("pt", "pq", "pa", "pclv")
TMP = ("tendency_tmp_t", "tendency_tmp_q", "tendency_tmp_a", "tendency_tmp_cld")
LOC = ("tendency_loc_t", "tendency_loc_q", "tendency_loc_a", "tendency_loc_cld")
ADV = ("t", "q", "a", "clv")                 # the members of cloudsc_advance_t, in the order of STATE
NSPEC = 4                                     # ql, qi, qr, qs: the fifth (vapour) plane is never written
STATES = ["W", "M", "shipped", "ncldtop40", "ncldtop138", "klev3", "klev274", "aerosol_W", "ptsphy_7200"]
# tail of 36 lanes | narrow blocks (packed by default on the device) | two sub-blocks per block, columns repeat
SHAPES = [(100, 64), (100, 16), (300, 128)]
OUTPUTS = {"all": ca.OUTPUTS_ALL, "surface": ca.OUTPUTS_SURFACE}
CANARY = 0x5D                                 # what must keep its bytes
NAMES = fs.NAMES


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def dataset(name, ds, scenarios):
    """A state of form_state_cases, or the shipped state itself."""
    if name == "shipped":
        return ds
    return fs.dataset(name, ds, scenarios)


def two_lines(x, tmp, loc, ptsphy, dtype):
    """The definition on arrays of one shape, in `dtype`."""
    dt = dtype(ptsphy)
    x, tmp, loc = (np.ascontiguousarray(a, dtype=dtype) for a in (x, tmp, loc))
    a = np.multiply(dt, tmp, dtype=dtype)
    x0 = np.add(x, a, dtype=dtype)
    b = np.multiply(dt, loc, dtype=dtype)
    return np.add(x0, b, dtype=dtype)


def advanced(inputs, loc, ptsphy, dtype):
    """{state member: [..][n]} after one step: inputs and loc are {name: [..][n]} in columns; pclv keeps its
    vapour plane."""
    out = {}
    for x, t, l in zip(STATE, TMP, LOC):
        sl = slice(0, NSPEC if x == "pclv" else None)      # pclv: the four condensate planes
        new = two_lines(inputs[x][sl], inputs[t][sl], loc[l][sl], ptsphy, dtype)
        if x == "pclv":
            new = np.concatenate([new, np.ascontiguousarray(inputs[x][NSPEC:], dtype=dtype)], axis=0)
        out[x] = new
    return out


def wrap(cols, ngptot):
    """Template columns [..][klon] as the ngptot columns of a run: column g is template column g % klon."""
    return np.ascontiguousarray(cols[..., np.arange(ngptot) % cols.shape[-1]])


_expected = {}


def expected(oracle_mod, name, s, precision):
    """({state member: [..][klon]}, {other output: [..][klon]}) of one advancing step on the state in fp64 or mixed:
    the oracle's outputs, then the two lines in float64; mixed = float32 of that on float64(float32 inputs)."""
    key = (name, precision)
    if key not in _expected:
        assert fs.NGPTOT == s.klon
        if precision == ca.FP64:
            src, out = s, fs.oracle_outputs(oracle_mod, name, s)
        else:
            src = mx.rounded_inputs(s)
            st, _ = oracle_mod.run_oracle(src, fs.NGPTOT, fs.ORACLE_NPROMA)
            out = {k: np.ascontiguousarray(ca.blocks_to_columns(st.arrays[k], fs.NGPTOT)) for k in NAMES}
        new = advanced(src.inputs, out, s.params["ptsphy"], np.float64)
        other = {k: out[k] for k in NAMES if k not in LOC}
        if precision == ca.MIXED:
            with np.errstate(over="ignore", under="ignore"):
                new = {k: a.astype(np.float32) for k, a in new.items()}
                other = {k: a.astype(np.float32) for k, a in other.items()}
        for a in list(new.values()) + list(other.values()):
            a.setflags(write=False)
        _expected[key] = (new, other)
    return _expected[key]


def surface_row(name, a):
    """What an OUTPUTS_SURFACE set holds of a profile of the four surface fluxes: its last row."""
    return a[-1] if name in ca.SURFACE_FLUX_FIELDS else a


def adv_struct(arrays_or_ptrs):
    """An Advance from {state member: array | address}."""
    adv = ca.Advance()
    for m, x in zip(ADV, STATE):
        v = arrays_or_ptrs[x]
        setattr(adv, m, v.ctypes.data if isinstance(v, np.ndarray) else v)
    return adv
