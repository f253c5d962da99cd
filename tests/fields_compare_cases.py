"""TEST INFRASTRUCTURE ONLY -- cases and the restatement of the field set comparison
(cloudsc_fields_compare / cloudsc_cpu_fields_compare), in NumPy and fractions.Fraction:

    for every member, row and global column g < ngptot, v = double(a[g // anp][row][g % anp]) and
    r = double(b[g // bnp][row][g % bnp]):  min v, max v, max |v - r|, sum |v - r|, sum |r| (exact rationals
    here), the number of elements whose bits differ and the smallest (g, row) of them

Nothing here calls the library under test.

The bound on a double-double sum.  dd_add (csrc/cloudsc_internal.h) is a TwoSum of the high parts (exact)
followed by three rounded operations on quantities no larger than the running sum's last-place unit: each
rounds by at most 2^-53 of a value below 2^-51 of the sum, so one addition leaves the pair within 2^-104 of
the sum it holds.  All terms are non-negative, so every running sum is at most the total F; adding n
elements and combining at most n partial records is at most 2n additions: |hi + lo - F| <= n * 2^-103 * F,
inside the n * 2^-100 * F asserted here."""
from fractions import Fraction

import numpy as np

import cloudsc_amd as ca
import fields_convert_cases as fc

KLEV = fc.KLEV
# (ngptot, NPROMA a, NPROMA b) at KLEV 3, every member
SHAPES = list(fc.SHAPES) + [(1, 1, 64), (333, 300, 64)]
# the same at KLEV 137, the output members (species: 685 rows)
TALL_KLEV = 137
TALL_SHAPES = [(1000, 64, 24), (1000, 1000, 64)]
OUTPUTS = [k for _, k in ca.VALIDATED]
STORAGE = fc.STORAGE
STORAGE_IDS = ["dd", "df", "fd", "ff"]
SEED = 20260519
NAN_A = bytes([0xFF])      # every byte of a's padding lanes: a NaN with all payload bits set (ktype: -1)
NAN_B = np.nan             # b's padding lanes: the default quiet NaN (ktype: -2), another word than a's


def encoded(name, rows, ngptot):
    """[rows][ngptot] distinct values exact in float: fields_convert_cases.encoded where it reaches, else
    (member % 16, row, column) in 4 + 10 + 10 bits."""
    if ngptot <= 256:
        return fc.encoded(name, rows, ngptot)
    assert rows < 1024 and ngptot <= 1024
    m = fc.MEMBERS.index(name) % 16
    return (m << 20) + (np.arange(rows, dtype=np.int64)[:, None] << 10) + np.arange(ngptot, dtype=np.int64)[None, :]


def fill_set(hs, cols, pad):
    """cols: {member: [rows][ngptot]} into the HostSet's block layout, `pad` in the padding lanes."""
    for n in hs.names:
        dt = hs.arrays[n].dtype
        p = pad
        if dt == np.int32:
            p = -1 if isinstance(pad, bytes) else -2
        hs.arrays[n][...] = fc.to_blocks(cols[n].astype(dt), hs.nproma, dt, p)
    return hs


def planted(names, klev, ngptot, rng):
    """(member, row, global column) positions where b is made to differ from a: column 0 row 0, the last
    active lane (of a partial last block, where the shape has one) in its last row, ktype, and seeded
    others.  The first real member's (row 0, column 0) is the +0 / -0 pair, handled by make_pair."""
    real = [n for n in names if n != "ktype"]
    pos = [(real[1 % len(real)], 0, 0)]
    tall = max(real, key=lambda n: fc.rows_of(n, klev))
    pos.append((tall, fc.rows_of(tall, klev) - 1, ngptot - 1))
    if "ktype" in names:
        pos.append(("ktype", 0, ngptot // 2))
    for _ in range(6):
        n = real[int(rng.integers(len(real)))]
        pos.append((n, int(rng.integers(fc.rows_of(n, klev))), int(rng.integers(ngptot))))
    return pos


def make_pair(ngptot, anp, bnp, klev, ap, bp, names=None, seed=SEED, plant=True):
    """Two HostSets of the same encoded values in their own blockings and storage types, different NaN
    words in their padding lanes, b changed at the planted positions.  Returns (a, b, positions)."""
    names = list(fc.MEMBERS if names is None else names)
    rng = np.random.default_rng(seed)
    ca_cols = {n: encoded(n, fc.rows_of(n, klev), ngptot).astype(np.float64) for n in names}
    cb_cols = {n: v.copy() for n, v in ca_cols.items()}
    pos = []
    if plant:
        pos = planted(names, klev, ngptot, rng)
        for n, row, g in pos:
            if n == "ktype":
                cb_cols[n][row, g] += 1 + int(rng.integers(5))
            else:   # an odd multiple of 1 / 64 below 2^14: exact in float, never the integer it replaces
                cb_cols[n][row, g] = (2 * int(rng.integers(1 << 19)) + 1) / 64.0
        zero = [n for n in names if n != "ktype"][0]
        ca_cols[zero][0, 0] = 0.0
        cb_cols[zero][0, 0] = -0.0
        pos.append((zero, 0, 0))
    a = fill_set(fc.HostSet(ngptot, anp, klev, ap, names=names), ca_cols, NAN_A)
    b = fill_set(fc.HostSet(ngptot, bnp, klev, bp, names=names), cb_cols, NAN_B)
    return a, b, pos


def exact_sum(x):
    """The exact sum of a float64 array as a Fraction (None if it holds a NaN or an infinity)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if not np.all(np.isfinite(x)):
        return None
    small = (x == np.floor(x)) & (np.abs(x) < 2.0 ** 31)
    assert x.size < 2 ** 31
    total = Fraction(int(x[small].astype(np.int64).sum()))
    for t in x[~small]:
        total += Fraction(float(t))
    return total


def restate(a, b, names=None):
    """{member: record} of a against b: compared, mismatches, first (column, row), min, max, maxerr as
    floats, errsum / refsum as exact Fractions (None where a NaN enters)."""
    out = {}
    for n in (a.names if names is None else names):
        A, B = fc.to_columns(a.arrays[n], a.ngptot), fc.to_columns(b.arrays[n], b.ngptot)
        v, r = A.astype(np.float64), B.astype(np.float64)
        with np.errstate(invalid="ignore"):
            d = np.abs(v - r)
        if A.dtype == B.dtype:
            differ = fc.bits(A) != fc.bits(B)
        else:
            differ = fc.bits(v) != fc.bits(r)
        rows = A.shape[0]
        first = (-1, -1)
        if differ.any():
            rr, gg = np.nonzero(differ)
            key = int((gg.astype(np.int64) * rows + rr).min())
            first = (key // rows, key % rows)
        out[n] = {"compared": rows * a.ngptot, "mismatches": int(np.count_nonzero(differ)), "first": first,
                  "min": float(np.fmin.reduce(v, axis=None)), "max": float(np.fmax.reduce(v, axis=None)),
                  "maxerr": float(np.fmax.reduce(d, axis=None, initial=0.0)),
                  "errsum": exact_sum(d), "refsum": exact_sum(np.abs(r))}
    return out


def dbits(x):
    return np.float64(x).view(np.uint64)


def exact_fields(d):
    """The fields of a FieldDiff that must not depend on grouping, thread count, grid or blocking."""
    s = d.stats
    return (d.compared, d.mismatches, d.first_column, d.first_row, int(dbits(s.minval)), int(dbits(s.maxval)),
            int(dbits(s.maxerr)))


def dd_value(hi, lo):
    return Fraction(hi) + Fraction(lo)


def assert_sum(hi, lo, F, n, what):
    """hi + lo within n * 2^-100 * F of the exact sum F, and hi its correctly rounded double."""
    assert not np.isnan(hi) and not np.isnan(lo), what
    assert abs(dd_value(hi, lo) - F) <= n * Fraction(1, 2 ** 100) * F, (what, hi, lo, float(F))
    assert hi == float(F), (what, hi, float(F))


def check_against_restatement(diffs, exp):
    """diffs: the FieldDiff array of a call; exp: restate(...).  Members not in exp must be skipped records."""
    for m, n in enumerate(fc.MEMBERS):
        d = diffs[m]
        s = d.stats
        if n not in exp:
            assert (d.compared, d.mismatches, d.first_column, d.first_row) == (0, 0, -1, -1), n
            assert (s.minval, s.maxval, s.maxerr, s.errsum, s.refsum, s.errsum_lo, s.refsum_lo) == (
                np.finfo(np.float64).max, -np.finfo(np.float64).max, 0.0, 0.0, 0.0, 0.0, 0.0), n
            continue
        e = exp[n]
        assert d.compared == e["compared"], n
        assert d.mismatches == e["mismatches"], (n, d.mismatches, e["mismatches"])
        assert (d.first_column, d.first_row) == e["first"], (n, d.first_column, d.first_row, e["first"])
        assert dbits(s.minval) == dbits(e["min"]) and dbits(s.maxval) == dbits(e["max"]), (n, s.minval, s.maxval)
        assert dbits(s.maxerr) == dbits(e["maxerr"]), (n, s.maxerr, e["maxerr"])
        assert_sum(s.errsum, s.errsum_lo, e["errsum"], e["compared"], n + " errsum")
        assert_sum(s.refsum, s.refsum_lo, e["refsum"], e["compared"], n + " refsum")


def new_diffs():
    return (ca.FieldDiff * len(fc.MEMBERS))()
