"""TEST INFRASTRUCTURE ONLY -- the per-column parameter multipliers (SPP) for the tests of
cloudsc_*_run_spp: the five slots, the four multiplier tuples, which column carries which tuple, how the
host scales a parameter set by a tuple in each precision, and how the expected outputs of a mixed-tuple run
are put together from one ordinary step per tuple.  Nothing here calls the library under test."""
import numpy as np

import cloudsc_amd as ca

# the members of cloudsc_spp_t, in order
SLOTS = ("ramid", "rcldiff", "rclcrit", "rlcritsnow", "rpecons")
# the cloudsc_params_t members a slot's multiplier scales
PARAMS_OF = {"ramid": ("ramid",), "rcldiff": ("rcldiff",), "rclcrit": ("rclcrit_sea", "rclcrit_land"),
             "rlcritsnow": ("rlcritsnow",), "rpecons": ("rpecons",)}
TUPLES = (
    (1.0, 1.0, 1.0, 1.0, 1.0),
    (0.7531, 1.2519, 0.5017, 1.2483, 0.7469),
    (1.1203, 0.7487, 1.4989, 0.7523, 1.2511),
    (1.0, 1.2519, 1.0, 0.7523, 1.0),
)
NTUPLES = len(TUPLES)


def group(g):
    """The tuple of global column g: every wave and every 16-column block holds all four."""
    g = np.asarray(g)
    return (7 * g + g // 16) % 4


def only(slot, t):
    """Tuple t with every slot but `slot` at 1."""
    return tuple(x if s == slot else 1.0 for s, x in zip(SLOTS, TUPLES[t]))


def stored(x, precision):
    """The multiplier as the fields hold it: a double in fp64, a float in fp32 and mixed."""
    return ca.storage_dtype(precision)(x)


def scaled_params(params, tup, precision):
    """The parameter dict of the ordinary step that equals the SPP step under the one tuple `tup`: p.n * x in
    double for fp64; for mixed the same with x the stored float widened; for fp32 the float product widened."""
    p = dict(params)
    for slot, x in zip(SLOTS, tup):
        for n in PARAMS_OF[slot]:
            if precision == ca.FP32:
                p[n] = float(np.float32(p[n]) * np.float32(x))
            else:
                p[n] = float(np.float64(p[n]) * np.float64(stored(x, precision)))
    return p


def scaled_dataset(ds, tup, precision):
    s = ds.copy()
    s.params = scaled_params(ds.params, tup, precision)
    s.reference = {}
    return s


def multiplier_fields(ngptot, nproma, precision, tuples=TUPLES, pad=None):
    """{slot: [nblocks][nproma]} in the storage type, column g holding tuples[group(g)]; the padding lanes of a
    partial last block hold `pad` (a NaN by default: a read of one shows in the outputs)."""
    dt = ca.storage_dtype(precision)
    nb = ca.nblocks_of(ngptot, nproma)
    g = np.arange(nb * nproma).reshape(nb, nproma)
    t = np.asarray(tuples, dtype=np.float64)[group(g) % len(tuples)]          # [nb][nproma][5]
    out = {}
    for i, s in enumerate(SLOTS):
        a = t[..., i].astype(dt)
        a[g >= ngptot] = np.nan if pad is None else pad
        out[s] = np.ascontiguousarray(a)
    return out


def uniform_fields(ngptot, nproma, precision, tup):
    return multiplier_fields(ngptot, nproma, precision, tuples=(tup,))


def spp_struct(arrays):
    """A ca.Spp pointing at host arrays {slot: array or None}."""
    s = ca.Spp()
    for n in SLOTS:
        a = arrays.get(n)
        setattr(s, n, a.ctypes.data if a is not None else None)
    return s


def select_columns(per_tuple, ngptot, names):
    """{name: [..][ngptot]} taking column g from per_tuple[group(g)][name] (column-last arrays)."""
    grp = group(np.arange(ngptot))
    out = {}
    for n in names:
        a = np.array(per_tuple[0][n], copy=True)
        for t in range(1, len(per_tuple)):
            m = grp == t
            a[..., m] = np.asarray(per_tuple[t][n])[..., m]
        out[n] = a
    return out


def expected_mixed_tuples(step, ds, ngptot, precision, names, tuples=TUPLES):
    """The expected outputs of a run whose column g carries tuples[group(g)]: step(dataset) -> {name:
    [..][ngptot]} is run once per tuple on the host-scaled parameter set, and each column is taken from the
    run of its tuple."""
    per_tuple = [step(scaled_dataset(ds, t, precision)) for t in tuples]
    return select_columns(per_tuple, ngptot, names)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def changed_columns(a, b):
    """Columns (last axis) in which any element of two column-last arrays differs in its bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint64 if a.itemsize == 8 else np.uint32
    d = a.view(u) != b.view(u)
    return np.flatnonzero(d.reshape(-1, d.shape[-1]).any(axis=0))
