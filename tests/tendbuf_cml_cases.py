"""TEST INFRASTRUCTURE ONLY -- the cumulative tendency buffer (BUFFER_CML) for the tests of
cloudsc_*_run_tendbuf_cml and cloudsc_*_fields_accumulate_tendbuf: where its four members sit, what it
holds before a run, and what it must hold after one, restated in NumPy.  Nothing here calls the library
under test."""
import numpy as np

import cloudsc_amd as ca
import tendbuf_cases as tb

CML = ("t", "q", "a", "cld")
LOC_OF = {"t": "tendency_loc_t", "q": "tendency_loc_q", "a": "tendency_loc_a", "cld": "tendency_loc_cld"}
SPECIES = ca.NCLV - 1          # ql, qi, qr, qs are accumulated; the fifth plane (vapour) is left alone
QR = 2

# first plane of (t, q, a, cld) in BUFFER_CML; cld takes five consecutive planes, the fifth never touched
REFERENCE = {8: (0, 2, 1, 3), 11: (0, 2, 1, 3)}          # CLOUDSC_TENDBUF_T/Q/A/CLD = 0, 2, 1, 3
PERMUTED = {8: (6, 7, 0, 1), 11: (9, 0, 10, 2)}


def layout(order, tend_planes):
    return dict(zip(CML, (REFERENCE if order == "reference" else PERMUTED)[tend_planes]))


def background(shape, dtype):
    """Every element of a buffer before the seven planes are filled: a cycle of -0.0, a NaN with a payload,
    a sentinel bit pattern and 1.5 -- an `x + 0` anywhere it does not belong changes the first two."""
    u = np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32
    neg0 = np.array(-0.0, dtype).view(u)
    nan = (np.array(np.nan, dtype).view(u) | u(0x5A5)) | (u(1) << u(8 * np.dtype(dtype).itemsize - 1))
    sent = u(0xA5A5A5A5A5A5A5A5 & ((1 << (8 * np.dtype(dtype).itemsize)) - 1))
    one5 = np.array(1.5, dtype).view(u)
    cyc = np.array([neg0, nan, sent, one5], dtype=u)
    n = int(np.prod(shape))
    return np.resize(cyc, n).reshape(shape).view(dtype)


def seeded_values(shape, dtype, seed):
    """Mixed signs, magnitudes 1e-12 .. 1e-2 (the tendencies' range and around it) with full mantissas, so
    that adding a tendency rounds; a few exact zeros of both signs."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(1.0, 10.0, shape) * 10.0 ** rng.integers(-12, -2, shape) * rng.choice([-1.0, 1.0], shape)
    z = rng.random(shape)
    v[z < 0.01] = 0.0
    v[(z >= 0.01) & (z < 0.02)] = -0.0
    return v.astype(dtype)


def touched_mask(shape, lay, ngptot):
    """True at the elements a run may change: the seven planes, the lanes of real columns."""
    nb, _, _, nproma = shape
    m = np.zeros(shape, dtype=bool)
    for b in range(nb):
        cols = min(nproma, ngptot - b * nproma)
        for k in CML:
            if lay[k] < shape[1]:          # (a member that lives in another array: not in this one)
                m[b, lay[k]:lay[k] + (SPECIES if k == "cld" else 1), :, :cols] = True
    return m


def make_buffer(nb, tend_planes, klev, nproma, dtype, lay, ngptot, seed, zero=False):
    buf = background((nb, tend_planes, klev, nproma), dtype).copy()
    m = touched_mask(buf.shape, lay, ngptot)
    buf[m] = 0.0 if zero else seeded_values(buf.shape, dtype, seed)[m]
    return buf


def bind(lay, buf):
    """A TendCml pointing at its planes of buf."""
    _, _, klev, nproma = buf.shape
    c = ca.TendCml()
    for k in CML:
        setattr(c, k, buf.ctypes.data + lay[k] * klev * nproma * buf.itemsize)
    return c


def loc_planes(loc, k):
    """[nb][n][klev][nproma]: the planes of block-layout tendency_loc_<k> that are accumulated."""
    a = np.asarray(loc[LOC_OF[k]])
    return a[:, :SPECIES] if k == "cld" else a[:, None]


def expected(before, lay, ngptot, loc, add):
    """The buffer after one accumulation: add(cml_old, loc) at the touched elements, every other byte as
    before.  loc: {tendency_loc_*: block-layout array}; add: the precision's rule."""
    out = before.copy()
    nb, _, _, nproma = before.shape
    for k in CML:
        if lay[k] >= before.shape[1]:
            continue
        n = SPECIES if k == "cld" else 1
        l = loc_planes(loc, k)
        for b in range(nb):
            cols = min(nproma, ngptot - b * nproma)
            sl = (b, slice(lay[k], lay[k] + n), slice(None), slice(0, cols))
            out[sl] = add(before[sl], l[b, :, :, :cols])
    return out


def add_storage(old, loc):
    """fp64, fp32 and the separate pass: one add in the storage type."""
    return (old + loc.astype(old.dtype)).astype(old.dtype)


def add_mixed(old, loc64):
    """The fused mixed form: float32(float64(cml) + loc64)."""
    return (old.astype(np.float64) + np.asarray(loc64, dtype=np.float64)).astype(np.float32)


def same_bits(a, b):
    return np.array_equal(tb.bits(a), tb.bits(b))
