"""TEST INFRASTRUCTURE ONLY -- cases and the NumPy restatement of the layout conversion
(cloudsc_fields_convert_layout / cloudsc_cpu_fields_convert_layout):

    L[g, r] = B[g // np, r, g % np],  g < ngptot        (L: LAYOUT_LEVELS, B: LAYOUT_BLOCKED)

with the conversion of fields_convert_cases.py.  The data is random bit patterns: no physics state is
needed, so any klev works.  Nothing here calls the library under test."""
import zlib

import numpy as np

import cloudsc_amd as ca
import fields_convert_cases as fc

B, L = ca.LAYOUT_BLOCKED, ca.LAYOUT_LEVELS

# (ngptot, NPROMA of the blocked side, klev).  NGPTOT crosses the wave (64) and the tile (256) edges and
# leaves a partial last block; klev 3 / 15 / 16 / 17 / 137 give rows of 3/4/15, 15/16/75, 16/17/80, 17/18/85
# and 137/138/685: on, below and above the edge of a 16-row chunk.  Not the full product: every value of
# each axis with at least two values of the others.
SHAPES = [(1, 64, 3), (1, 5, 17),
          (63, 64, 15), (63, 16, 16),
          (64, 64, 16), (64, 5, 3),
          (65, 64, 17), (65, 16, 15), (65, 300, 137),
          (255, 64, 3), (255, 300, 16),
          (257, 16, 17), (257, 5, 15),
          (300, 64, 137), (300, 16, 3), (300, 5, 17), (300, 300, 15), (300, 64, 16)]
STORAGE = fc.STORAGE
STORAGE_IDS = ["d2d", "d2f", "f2d", "f2f"]
# every shape with two of the four storage pairs, every pair with nine shapes
CASES = [(s, STORAGE[(i + j) % 4]) for i, s in enumerate(SHAPES) for j in (0, 2)]
CASE_IDS = ["%d-%d-%d-%s" % (s + (STORAGE_IDS[STORAGE.index(p)],)) for s, p in CASES]

INPUTS = list(ca.INPUT_FIELDS) + list(ca.INOUT_FIELDS)
OUTPUTS = [n for n in fc.MEMBERS if n not in ca.INPUT_FIELDS]


def rows_of(name, klev, outputs=ca.OUTPUTS_ALL):
    if outputs == ca.OUTPUTS_SURFACE and name in ca.SURFACE_FLUX_FIELDS:
        return 1
    return fc.rows_of(name, klev)


def random_columns(name, rows, ngptot, dt, seed=0):
    """[rows][ngptot] of dtype dt.  float32 and int32: random bits.  float64: random bits in the even
    columns; in the odd ones random float bits widened, with random bits below the float's mantissa, so
    that a narrowing copy has in-range values to round."""
    rng = np.random.default_rng([zlib.crc32(name.encode()), rows, ngptot, seed])
    if np.dtype(dt).itemsize == 4:
        return rng.integers(0, 1 << 32, size=(rows, ngptot), dtype=np.uint64).astype(np.uint32).view(dt)
    bits = rng.integers(0, 1 << 63, size=(rows, ngptot), dtype=np.uint64) << np.uint64(1)
    bits |= rng.integers(0, 2, size=(rows, ngptot), dtype=np.uint64)
    f = rng.integers(0, 1 << 32, size=(rows, ngptot), dtype=np.uint64).astype(np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        wide = f.astype(np.float64).view(np.uint64) | (bits & np.uint64((1 << 29) - 1))
    bits[:, 1::2] = wide[:, 1::2]
    return bits.view(np.float64)


class HostSet:
    """Host arrays of a field set in either layout, each followed by fc.GUARD elements; the whole buffer
    (`full[name]`) starts as the sentinel byte pattern.  arrays[name] is [nb][rows][nproma] (BLOCKED) or
    [ngptot][rows] (LEVELS, nproma 0)."""

    def __init__(self, layout, ngptot, nproma, klev, precision, names=None, outputs=ca.OUTPUTS_ALL):
        assert (nproma == 0) == (layout == L)
        self.layout, self.ngptot, self.nproma, self.klev, self.precision = layout, ngptot, nproma, klev, precision
        self.outputs = outputs
        self.names = list(fc.MEMBERS if names is None else names)
        self.full, self.arrays = {}, {}
        for n in self.names:
            dt, rows = fc.dtype_of(n, precision), rows_of(n, klev, outputs)
            shape = (ngptot, rows) if layout == L else (ca.nblocks_of(ngptot, nproma), rows, nproma)
            size = int(np.prod(shape))
            buf = np.empty(size + fc.GUARD, dtype=dt)
            buf.view(np.uint8)[...] = fc.SENTINEL_BYTE
            self.full[n] = buf
            self.arrays[n] = buf[:size].reshape(shape)

    def rows(self, n):
        return rows_of(n, self.klev, self.outputs)

    def fill_random(self, seed=0):
        for n in self.names:
            self.set_columns(n, random_columns(n, self.rows(n), self.ngptot, self.arrays[n].dtype, seed))
        return self

    def set_columns(self, n, cols):
        """arrays[n] from [rows][ngptot]; the padding lanes of a blocked set get fc.POISON."""
        if self.layout == L:
            self.arrays[n][...] = cols.T
        else:
            self.arrays[n][...] = fc.to_blocks(cols, self.nproma, self.arrays[n].dtype, fc.POISON)

    def columns(self, n):
        """[rows][ngptot]"""
        return self.arrays[n].T if self.layout == L else fc.to_columns(self.arrays[n], self.ngptot)

    def fields(self, names=None):
        f = ca.Fields()
        for n in (self.names if names is None else names):
            setattr(f, n, self.arrays[n].ctypes.data)
        return f

    def guard_intact(self, n):
        return bool(np.all(self.full[n][self.arrays[n].size:].view(np.uint8) == fc.SENTINEL_BYTE))

    def untouched(self, n):
        return bool(np.all(self.full[n].view(np.uint8) == fc.SENTINEL_BYTE))

    def like(self, layout=None, nproma=None, precision=None, names=None):
        """A sentinel-filled set of the same problem in another layout / blocking / precision."""
        layout = self.layout if layout is None else layout
        nproma = 0 if layout == L else (self.nproma if nproma is None else nproma)
        return HostSet(layout, self.ngptot, nproma, self.klev, self.precision if precision is None else precision,
                       self.names if names is None else names, self.outputs)


def expected(src, dst, n):
    """The NumPy restatement for one member: dst's whole array, sentinel bytes in the padding lanes of a
    blocked destination."""
    dt = dst.arrays[n].dtype
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        cols = src.columns(n).astype(dt)
    if dst.layout == L:
        return np.ascontiguousarray(cols.T)
    return fc.to_blocks(cols, dst.nproma, dt, bytes([fc.SENTINEL_BYTE]))


def same_values(got, exp, moved_bits):
    """Raw bits; after a narrowing or widening conversion a NaN only has to be a NaN where one is expected
    (its payload is the converting hardware's)."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return False
    if moved_bits or got.dtype.kind != "f":
        return np.array_equal(fc.bits(got), fc.bits(exp))
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(fc.bits(got)[~nan], fc.bits(exp)[~nan])


def check_against_numpy(src, dst, names=None):
    """Every named member of dst is the restatement of src, padding lanes and guard margin still the sentinel."""
    moved = fc.dtype_of("pt", src.precision).itemsize == fc.dtype_of("pt", dst.precision).itemsize
    for n in (dst.names if names is None else names):
        assert same_values(dst.arrays[n], expected(src, dst, n), moved), (n, "differs from the NumPy restatement")
        assert dst.guard_intact(n), (n, "guard margin written")


def same_sets(a, b, names=None):
    """Two sets of one shape hold the same bytes in every named buffer, guard margins included."""
    for n in (a.names if names is None else names):
        assert np.array_equal(a.full[n].view(np.uint8), b.full[n].view(np.uint8)), n
