"""Field layouts for the stride / offset / chunk tests (test infrastructure only).

make_view(dense, layout) places a dense array's values in a larger buffer
under one of the named layouts and returns (buffer, view): `buffer` is a flat
array pre-filled with a sentinel bit pattern, `view` a numpy view of it with
the dense array's shape and values.  Whatever a codec writes outside the view
shows as a changed sentinel (check_guard).  All comparisons are on raw bits
(the arrays seen as unsigned integers), so NaN payloads and -0 compare exactly.

Strides below are in elements, zfp order (x, the last numpy axis, first):

  dense        1, nx, nx ny, ...
  pad4         unit x; every other stride rounded up to a multiple of 4 plus 4
               (rows stay 16-byte aligned: the kernels' vector row path)
  pad3         unit x; every other stride rounded up to a multiple of 4 plus 3
               (rows lose their alignment: the scalar row path)
  shift1       dense, but the view starts one element into an aligned buffer
               (the base pointer is not 16-byte aligned)
  interleaved  x stride 2, the other axes dense over the doubled rows
  transposed   storage in reversed axis order (x slowest); 2D and up
  rev_x        dense with the x stride negated
  rev_outer    dense with the outermost stride negated
  rev_all      dense with every stride negated
  rev_y        dense with the y stride negated (unit x stride); 2D and up

For negative strides view.ctypes.data is the address of logical element 0,
which is what the C API and the oracle take as the field pointer.
"""
import numpy as np
from numpy.lib.stride_tricks import as_strided

LAYOUTS = ["dense", "pad4", "pad3", "shift1", "interleaved", "transposed", "rev_x", "rev_outer", "rev_all", "rev_y"]
SENTINEL_BYTE = 0xA5
# the smallest shapes with a partial block on every axis and more than one wave
# of blocks (64 blocks a wave in 1D-3D, 16 in 4D): 66, 80, 72 and 24 blocks
SHAPES = {1: (263,), 2: (30, 37), 3: (10, 14, 22), 4: (5, 6, 7, 9)}
FIXED_RATE = {1: 8, 2: 8, 3: 12, 4: 6}  # the fixed-rate mode of each dimensionality
# Chunk boxes of those shapes, (first, end) per zfp axis (x first, ends exclusive):
#   inside   block-aligned origin, an end inside the field that is no multiple of 4
#            (as far as the short axes of the 4D shape allow)
#   edge     runs to the field's far edge on every axis: partial blocks
#   odd_x    origin off a multiple of 4 on x only
#   odd_all  origin off a multiple of 4 on every axis
#   one      a single (partial, far-corner) block
CHUNK_BOXES = {
    1: {"inside": [(8, 150)], "edge": [(200, 263)], "odd_x": [(5, 131)], "odd_all": [(253, 263)], "one": [(260, 263)]},
    2: {"inside": [(4, 22), (8, 19)], "edge": [(20, 37), (12, 30)], "odd_x": [(6, 30), (4, 21)],
        "odd_all": [(6, 30), (3, 17)], "one": [(36, 37), (28, 30)]},
    3: {"inside": [(4, 18), (4, 10), (0, 7)], "edge": [(8, 22), (4, 14), (4, 10)], "odd_x": [(2, 19), (4, 12), (0, 8)],
        "odd_all": [(2, 19), (1, 11), (3, 9)], "one": [(20, 22), (12, 14), (8, 10)]},
    4: {"inside": [(4, 7), (0, 6), (0, 5), (0, 3)], "edge": [(4, 9), (4, 7), (0, 6), (0, 5)],
        "odd_x": [(1, 8), (0, 7), (4, 6), (0, 4)], "odd_all": [(1, 8), (2, 6), (1, 5), (1, 4)],
        "one": [(8, 9), (4, 7), (4, 6), (4, 5)]},
}
GUARD = 8  # sentinel elements before and after the span (8 elements keep a 32-byte aligned start)


def layouts_for(ndim):
    return [l for l in LAYOUTS if ndim >= 2 or l not in ("transposed", "rev_y")]


def _up4(v):
    return (v + 3) // 4 * 4


def element_strides(shape, layout):
    """Strides in elements, zfp order (x first), of `layout` for a numpy `shape`."""
    n = list(reversed(shape))
    d = len(n)
    if layout not in layouts_for(d):
        raise ValueError("%s is not a %dD layout" % (layout, d))
    s = [1] * d
    for a in range(1, d):
        s[a] = s[a - 1] * n[a - 1]
    if layout in ("pad4", "pad3"):
        for a in range(1, d):
            s[a] = _up4(s[a - 1] * n[a - 1]) + (4 if layout == "pad4" else 3)
    elif layout == "interleaved":
        s = [2 * v for v in s]
    elif layout == "transposed":
        s[d - 1] = 1
        for a in range(d - 2, -1, -1):
            s[a] = s[a + 1] * n[a + 1]
    elif layout == "rev_x":
        s[0] = -s[0]
    elif layout == "rev_outer":
        s[d - 1] = -s[d - 1]
    elif layout == "rev_all":
        s = [-v for v in s]
    elif layout == "rev_y":
        s[1] = -s[1]
    return s


def uint_of(dtype):
    return np.dtype("u%d" % np.dtype(dtype).itemsize)


def bits(a):
    """`a` seen as unsigned integers of its item size (works on strided views)."""
    return a.view(uint_of(a.dtype))


def special_field(shape, dtype, rng):
    """Hard float values in any dimensionality: magnitudes from 1e-3 to 1e5 with
    NaN, +-Inf, +-0, denormals and +-max sprinkled in, and whole blocks of
    denormals, -0, 0 and NaN along x at the field's origin (as many of the four
    as the x extent holds)."""
    a = (rng.standard_normal(shape) * rng.choice([1e-3, 1.0, 1e5], size=shape)).astype(dtype)
    flat = a.reshape(-1)
    info = np.finfo(dtype)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, info.tiny, info.tiny / 4, -info.tiny / 8,
                         info.max, -info.max], dtype=dtype)
    idx = rng.choice(flat.size, size=max(1, flat.size // 40), replace=False)
    flat[idx] = rng.choice(specials, size=idx.size)
    lead = (slice(0, 4),) * (a.ndim - 1)
    for k, v in enumerate((info.tiny / 16, -0.0, 0.0, np.nan)):
        if 4 * k + 4 <= shape[-1]:
            a[lead + (slice(4 * k, 4 * k + 4),)] = v
    return a


def edge_ints(shape, dtype, rng, full_range):
    """Integers at the edge of their range.  full_range (reversible mode): uniform
    over the whole type with MIN, MAX, -1 and 0 sprinkled in.  Otherwise values
    spanning the documented lossy range, |x| < 2^30 (int32) or 2^62 (int64)."""
    info = np.iinfo(dtype)
    if full_range:
        a = rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, size=max(4, flat.size // 8), replace=False)
        flat[idx] = rng.choice(np.array([info.min, info.max, -1, 0], dtype=dtype), size=idx.size)
        return a
    lim = 1 << (info.bits - 2)
    a = rng.integers(-lim + 1, lim, size=shape, dtype=dtype)
    flat = a.reshape(-1)
    flat[:4] = [lim - 1, -lim + 1, 0, -1]
    return a


def _aligned_flat(size, dtype):
    """A flat array of `size` elements whose first byte is 64-byte aligned."""
    dtype = np.dtype(dtype)
    raw = np.empty(size * dtype.itemsize + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + size * dtype.itemsize].view(dtype)


def make_view(dense, layout, fill=True):
    """(buffer, view): `view` has dense's shape and dtype under `layout` inside the
    sentinel-filled flat `buffer`; it holds dense's values unless fill=False (then
    it is sentinel too: a fresh decode destination)."""
    shape, dtype = dense.shape, dense.dtype
    s = element_strides(shape, layout)
    n = list(reversed(shape))
    lo = sum((n[a] - 1) * s[a] for a in range(len(n)) if s[a] < 0)
    hi = sum((n[a] - 1) * s[a] for a in range(len(n)) if s[a] > 0)
    start = GUARD + (1 if layout == "shift1" else 0) - lo
    buffer = _aligned_flat(start + hi + 1 + GUARD, dtype)
    bits(buffer)[...] = int.from_bytes(bytes([SENTINEL_BYTE]) * dtype.itemsize, "little")
    view = as_strided(buffer[start:], shape=shape, strides=[v * dtype.itemsize for v in reversed(s)])
    if fill:
        view[...] = dense
    return buffer, view


def chunk_written(shape, box):
    """Boolean array of numpy `shape`: the elements a chunk decode of `box` writes.
    The chunk's blocks start at its origin in steps of 4 and each is clipped by
    the field, not by the chunk's end (the reference's decompress loops)."""
    m = np.zeros(shape, dtype=bool)
    sl = []
    for a in range(len(shape) - 1, -1, -1):  # numpy axis order: zfp axis a is numpy axis ndim-1-a
        f, e = box[a]
        n = shape[len(shape) - 1 - a]
        sl.append(slice(f, min(n, f + (e - f + 3) // 4 * 4)))
    m[tuple(sl)] = True
    return m


def zfp_strides(view):
    """view's strides in elements, zfp order, padded to four entries with 0."""
    st = [v // view.itemsize for v in reversed(view.strides)]
    return st + [0] * (4 - len(st))


def outside_mask(buffer, view, written=None):
    """Boolean mask over `buffer`: True where an element is not part of `view`
    (or, with `written` a boolean array of view's shape, not a marked element)."""
    idx = np.arange(buffer.size, dtype=np.int64)
    start = (view.ctypes.data - buffer.ctypes.data) // buffer.itemsize
    iv = as_strided(idx[start:], shape=view.shape, strides=[v // view.itemsize * 8 for v in view.strides])
    mask = np.ones(buffer.size, dtype=bool)
    mask[iv.ravel() if written is None else iv[written]] = False
    return mask


def guard_intact(buffer, view, written=None):
    """Every element of `buffer` outside `view` (or outside the `written` elements
    of it) still holds the sentinel."""
    sentinel = int.from_bytes(bytes([SENTINEL_BYTE]) * buffer.itemsize, "little")
    return bool(np.all(bits(buffer)[outside_mask(buffer, view, written)] == sentinel))
