"""TEST INFRASTRUCTURE ONLY -- cases and the NumPy restatement of the field set
conversion (cloudsc_fields_convert / cloudsc_cpu_fields_convert):

    dst[g // dnp][row][g % dnp] = dst_type( src[g // snp][row][g % snp] ),  g < ngptot

Nothing here calls the library under test."""
import numpy as np

import cloudsc_amd as ca

# (ngptot, src NPROMA, dst NPROMA)
SHAPES = [(150, 8, 64), (150, 64, 8), (150, 24, 64), (150, 64, 24), (100, 100, 64), (130, 1, 64), (64, 64, 64),
          (150, 32, 150)]
# (src precision, dst precision): double -> double, double -> float, float -> double, float -> float
STORAGE = [(ca.FP64, ca.FP64), (ca.FP64, ca.MIXED), (ca.MIXED, ca.FP64), (ca.FP32, ca.FP32)]
KLEV = 3
GUARD = 96                 # elements after each array that must keep the sentinel
SENTINEL_BYTE = 0x5A       # every byte of a destination before the conversion
POISON = -7.0              # the source's padding lanes: never to be copied anywhere

MEMBERS = list(ca.ALL_FIELDS)


def rows_of(name, klev):
    return {"2d": klev, "2dh": klev + 1, "3d": ca.NCLV * klev, "1d": 1}[ca.ALL_FIELDS[name]]


def dtype_of(name, precision):
    return np.dtype(np.int32) if name == "ktype" else np.dtype(ca.storage_dtype(precision))


def uint_of(dt):
    return np.uint64 if np.dtype(dt).itemsize == 8 else np.uint32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(uint_of(a.dtype))


def encoded(name, rows, ngptot):
    """[rows][ngptot] values that encode (member, row, global column) uniquely in 24 bits:
    exactly representable in float, so every storage pair carries them unchanged."""
    m = MEMBERS.index(name)
    assert m < 64 and rows < 1024 and ngptot <= 256
    return (m << 18) + (np.arange(rows, dtype=np.int64)[:, None] << 8) + np.arange(ngptot, dtype=np.int64)[None, :]


def to_blocks(cols, nproma, dt, fill):
    """[rows][ngptot] -> block layout [nb][rows][nproma] of dtype dt; `fill` (a value, or a byte pattern when
    given as bytes) stands in the padding lanes of the last block."""
    rows, ngptot = cols.shape
    nb = ca.nblocks_of(ngptot, nproma)
    flat = np.empty((rows, nb * nproma), dtype=dt)
    if isinstance(fill, bytes):
        flat.view(np.uint8)[...] = fill[0]
    else:
        flat[...] = fill
    flat[:, :ngptot] = cols
    return np.ascontiguousarray(flat.reshape(rows, nb, nproma).transpose(1, 0, 2))


def to_columns(blocks, ngptot):
    """block layout [nb][rows][nproma] -> [rows][ngptot]"""
    nb, rows, nproma = blocks.shape
    return blocks.transpose(1, 0, 2).reshape(rows, nb * nproma)[:, :ngptot]


class HostSet:
    """Host arrays of a field set in block layout, each followed by GUARD elements; the whole buffer
    (`full[name]`) starts as the sentinel byte pattern."""

    def __init__(self, ngptot, nproma, klev, precision, names=None):
        self.ngptot, self.nproma, self.klev, self.precision = ngptot, nproma, klev, precision
        self.names = list(MEMBERS if names is None else names)
        self.full, self.arrays = {}, {}
        nb = ca.nblocks_of(ngptot, nproma)
        for n in self.names:
            dt, rows = dtype_of(n, precision), rows_of(n, klev)
            buf = np.empty(nb * rows * nproma + GUARD, dtype=dt)
            buf.view(np.uint8)[...] = SENTINEL_BYTE
            self.full[n] = buf
            self.arrays[n] = buf[:nb * rows * nproma].reshape(nb, rows, nproma)

    def fill_encoded(self):
        for n in self.names:
            self.arrays[n][...] = to_blocks(encoded(n, rows_of(n, self.klev), self.ngptot), self.nproma,
                                            self.arrays[n].dtype, POISON)
        return self

    def fields(self, names=None):
        f = ca.Fields()
        for n in (self.names if names is None else names):
            setattr(f, n, self.arrays[n].ctypes.data)
        return f

    def guard_intact(self, n):
        return bool(np.all(self.full[n][self.arrays[n].size:].view(np.uint8) == SENTINEL_BYTE))


def expected_blocks(src_blocks, ngptot, dst_nproma, dst_dt):
    """The NumPy restatement for one member: the destination array, sentinel bytes in its padding lanes."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        cols = to_columns(src_blocks, ngptot).astype(dst_dt)
    return to_blocks(cols, dst_nproma, dst_dt, bytes([SENTINEL_BYTE]))


def check_against_numpy(src, dst, names=None):
    """Every named member of dst equals the restatement of src bit for bit, padding lanes and guard
    margin still the sentinel."""
    for n in (dst.names if names is None else names):
        exp = expected_blocks(src.arrays[n], src.ngptot, dst.nproma, dst.arrays[n].dtype)
        assert np.array_equal(bits(dst.arrays[n]), bits(exp)), (n, "differs from the NumPy restatement")
        assert dst.guard_intact(n), (n, "guard margin written")


def narrowing_edges():
    """fp64 values whose conversion to float exercises every rounding rule of the contract."""
    below_tiny = np.nextafter(np.float64(2.0 ** -126), np.float64(0.0))
    v = [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24,       # ties: to even downwards, to even upwards
         2.0 ** -150, 1.5 * 2.0 ** -150,               # half the smallest subnormal: tie to zero; above it: up
         below_tiny,                                   # the largest fp64 below 2^-126: rounds up to 2^-126
         3.5e38,                                       # beyond FLT_MAX: infinity
         0.0, -0.0, np.inf, -np.inf, np.nan]
    v += [-x for x in v[:6]]
    return np.array(v, dtype=np.float64)
