"""TEST INFRASTRUCTURE ONLY -- packed tendency buffers for the tests of the
"tendbuf" entry points: the reference's Fortran drivers' layout

    BUFFER(NPROMA, NLEV, planes, NGPBLKS)   ==   [nblocks][planes][klev][nproma] in C order

built and taken apart in NumPy.  Nothing here calls the library under test."""
import numpy as np

import cloudsc_amd as ca

# (ngptot, nproma) | what it exercises
SHAPES = [
    (300, 64),    # five blocks, a 44-column last block
    (200, 128),   # two sub-blocks per block in KSEG, partial last block
    (100, 16),    # packed narrow by default, a 4-column last block
    (70, 32),     # packed with cloudsc_debug_set_narrow_pack(1)
    (300, 300),   # KSEG only, flat
]
TMP = ("tendency_tmp_t", "tendency_tmp_a", "tendency_tmp_q", "tendency_tmp_cld")
LOC = ("tendency_loc_t", "tendency_loc_a", "tendency_loc_q", "tendency_loc_cld")
SENTINEL_TMP, SENTINEL_LOC = 0x5A, 0xA5   # every byte of a buffer before it is filled / run

# first plane of (t, a, q, cld) in BUFFER_TMP and BUFFER_LOC; cld takes 5 consecutive planes
REFERENCE = {8: ((0, 1, 2, 3), (0, 1, 2, 3)), 11: ((0, 1, 2, 3), (0, 1, 2, 3))}
PERMUTED = {8: ((6, 7, 5, 0), (6, 0, 7, 1)), 11: ((10, 0, 8, 2), (0, 10, 1, 5))}


def layout(order, tend_planes):
    """{member: first plane} for the eight tendency members."""
    tmp, loc = (REFERENCE if order == "reference" else PERMUTED)[tend_planes]
    out = dict(zip(TMP, tmp))
    out.update(zip(LOC, loc))
    return out


def nplanes(name):
    return ca.NCLV if name.endswith("_cld") else 1


def empty_buffer(nb, tend_planes, klev, nproma, dtype, sentinel):
    buf = np.empty((nb, tend_planes, klev, nproma), dtype=dtype)
    buf.view(np.uint8)[...] = sentinel
    return buf


def put(buf, plane, blocks, ngptot):
    """The valid lanes of a block-layout member ([nb][klev][np] or [nb][5][klev][np]) into its planes."""
    nb, _, klev, nproma = buf.shape
    a = np.asarray(blocks).reshape(nb, -1, klev, nproma)
    for b in range(nb):
        n = min(nproma, ngptot - b * nproma)
        buf[b, plane:plane + a.shape[1], :, :n] = a[b, :, :, :n]


def take(buf, plane, name):
    """A member's planes of a buffer as a block-layout array (a copy)."""
    nb, _, klev, nproma = buf.shape
    a = buf[:, plane:plane + nplanes(name)]
    return np.ascontiguousarray(a if name.endswith("_cld") else a[:, 0])


def bind(f, lay, buf_tmp, buf_loc):
    """Point the eight tendency members of the ctypes Fields f at their planes of the two buffers."""
    for names, buf in ((TMP, buf_tmp), (LOC, buf_loc)):
        _, _, klev, nproma = buf.shape
        for n in names:
            setattr(f, n, buf.ctypes.data + lay[n] * klev * nproma * buf.itemsize)


def untouched_mask(buf, lay, names, ngptot):
    """True where a run or a conversion must leave the buffer alone: planes no member of `names` is bound
    to, and the lanes past the last column."""
    nb, _, _, nproma = buf.shape
    m = np.ones(buf.shape, dtype=bool)
    for n in names:
        for b in range(nb):
            cols = min(nproma, ngptot - b * nproma)
            m[b, lay[n]:lay[n] + nplanes(n), :, :cols] = False
    return m


def is_sentinel(buf, mask, sentinel):
    return bool(np.all(buf.view(np.uint8).reshape(buf.shape + (buf.itemsize,))[mask] == sentinel))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.itemsize == 8 else np.uint32)
