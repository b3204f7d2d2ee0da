"""Codec parameter lists and the exponent-ladder field of the parameter sweep
(test infrastructure only; shared by the CPU and the GPU sweep tests).

  RATES / INT_RATES   fixed-rate modes, in bits per value
  PRECISIONS          fixed-precision modes
  TOLERANCES          fixed-accuracy modes
  EXPERT              (minbits, maxbits, maxprec, minexp) tuples
  ladder_field        a field whose blocks step through every exponent of the type

Header bits H of a block: float 9 (lossy) / 15 (reversible), double 12 / 19,
integers 0 / 5 or 6.  No case has maxbits < H: the reference's own budget
subtraction wraps there.
"""
import math

import numpy as np

from pyoracle import ZFP_MAX_BITS, ZFP_MIN_EXP

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
I32, I64 = np.dtype(np.int32), np.dtype(np.int64)

HEADER_BITS = {F32: 9, F64: 12}
HEADER_BITS_REVERSIBLE = {F32: 15, F64: 19}

_FRACTIONAL_RATES = [0.25, 0.5, 1.5, 2.75, 7.5, 15.99, 16.01, 31.5]
RATES = {
    F64: list(range(1, 65)) + _FRACTIONAL_RATES,
    F32: list(range(1, 35)) + [40, 48, 64, 80] + _FRACTIONAL_RATES,
}
_INT_RATES = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33]
INT_RATES = {I32: list(_INT_RATES), I64: _INT_RATES + [63, 64]}

PRECISIONS = {
    F64: list(range(1, 65)),
    F32: list(range(1, 33)) + [33, 40, 64],
}

_TOLERANCE_EXPONENTS = [-1074, -1073, -1022, -200, -150, -149, -127, -126, -100, -30, -10, -1, 0, 1, 10, 100, 127,
                        128, 1000, 1023]


def _expressible(k):
    """2^k is a double and zfp_stream_set_accuracy's minexp for it is in range."""
    try:
        t = math.ldexp(1.0, k)
    except OverflowError:
        return False
    return t > 0 and math.isfinite(t) and math.frexp(t)[1] - 1 >= ZFP_MIN_EXP


def _tolerances():
    # the accuracy mode takes a double whatever the field's type
    return [0.0] + [math.ldexp(1.0, k) for k in _TOLERANCE_EXPONENTS if _expressible(k)] + \
        [1e-3, 3.0, 0.75 * math.ldexp(1.0, -20)]  # not powers of two: minexp is a floor


TOLERANCES = {F32: _tolerances(), F64: _tolerances()}


def _expert(dtype):
    h, hr = HEADER_BITS[dtype], HEADER_BITS_REVERSIBLE[dtype]
    lossless, rev = ZFP_MIN_EXP, ZFP_MIN_EXP - 1
    t = [(1024, 1024, 20, lossless), (1024, 1024, 33, lossless), (512, 512, 31, -40), (100, 100, 12, lossless)]
    t += [(1, mb, 64, lossless) for mb in (h, h + 1, 63, 64, 65, 127, 128, 129, ZFP_MAX_BITS)]
    # fixed rate with an accuracy floor: small blocks stop at their precision and are padded
    t += [(1024, 1024, 64, -20), (2048, 2048, 64, 0)]
    t += [(mn, ZFP_MAX_BITS, 64, lossless) for mn in (64, 65, 2200, 9000, ZFP_MAX_BITS)]
    t += [(mn, mb, 64, rev) for mb in (hr + 1, 200, ZFP_MAX_BITS) for mn in (1, 300) if mn <= mb]
    t += [(1, ZFP_MAX_BITS, mp, me) for mp in (1, 31, 32, 33, 63) for me in (lossless, -20, 0, 100)]
    return t


EXPERT = {F32: _expert(F32), F64: _expert(F64)}


# ---------------- the ladder field ----------------
def ladder_exponents(dtype):
    """e_b of the ladder blocks: the exponent of each block's largest magnitude."""
    if np.dtype(dtype) == F32:
        return list(range(-149, 128))
    dense = [(-1074, -1010), (-110, -85), (-40, 40), (1000, 1023)]
    es = set()
    for lo, hi in dense:
        es.update(range(lo, hi + 1))
    for (_, hi), (lo, _) in zip(dense, dense[1:]):
        es.update(e for e in range(hi + 1, lo) if e % 32 == 0)
    return sorted(es)


def ladder_block(e, n, dtype, rng):
    """n values: one of magnitude exactly 2^e, the others uniform in +-2^e, a few
    at 2^(e-40) and a few at 0, signs mixed."""
    few = max(1, n // 16)
    v = np.ldexp(rng.uniform(-1.0, 1.0, n), e)
    pos = rng.permutation(n)
    v[pos[1:1 + few]] = np.ldexp(rng.choice([-1.0, 1.0], few), e - 40)
    v[pos[1 + few:1 + 2 * few]] = 0.0
    v = v.astype(dtype)
    v[np.abs(v) > np.ldexp(1.0, e)] = 0  # (rounding cannot exceed 2^e; kept as a guard)
    v[pos[0]] = np.ldexp(rng.choice([-1.0, 1.0]), e)
    return v


def special_blocks(n, dtype, rng):
    info = np.finfo(dtype)
    denormal = np.ldexp(1.0, info.minexp - 3)
    one_inf = rng.standard_normal(n)
    one_inf[n // 3] = np.inf
    pm_max = np.where(np.arange(n) % 2 == 0, info.max, -info.max)
    blocks = [np.zeros(n), -np.zeros(n), np.full(n, np.nan), one_inf, np.full(n, denormal), pm_max]
    return [b.astype(dtype) for b in blocks]


# block grids (zfp order, x first): the smallest of that form that holds the ladder
_GRID_HEAD = {1: (), 2: (13,), 3: (5, 7), 4: (3, 3, 5)}
_cache = {}


def ladder_field(dims, dtype, partial, grid=None):
    """The ladder blocks and the special blocks, shuffled with a fixed seed and
    scattered into a field of whole blocks (grid slots beyond the list hold
    further ladder blocks); with `partial`, one element cut off the far end of
    every axis.  `grid` (blocks per axis, x first) replaces the default grid; a
    smaller one holds the first blocks of the shuffled list.  Made once per
    argument tuple and read-only."""
    dtype = np.dtype(dtype)
    key = (dims, dtype, bool(partial), grid)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 * dims + dtype.itemsize)
    n = 4 ** dims
    exps = ladder_exponents(dtype)
    count = len(exps) + 6
    if grid is None:
        head = int(np.prod(_GRID_HEAD[dims], dtype=np.int64))
        grid = _GRID_HEAD[dims] + ((count + head - 1) // head,)
        total = int(np.prod(grid))
        assert total > 64 and total % 64 != 0, grid  # more than one wave, and a ragged last one
    total = int(np.prod(grid))
    assert len(grid) == dims
    blocks = [ladder_block(e, n, dtype, rng) for e in exps] + special_blocks(n, dtype, rng)
    blocks += [ladder_block(exps[(7 * i) % len(exps)], n, dtype, rng) for i in range(total - count)]
    order = np.random.default_rng(5).permutation(max(total, count))
    shape = tuple(4 * g for g in reversed(grid))
    a = np.empty(shape, dtype=dtype)
    for slot, idx in enumerate(np.ndindex(*reversed(grid))):
        a[tuple(slice(4 * i, 4 * i + 4) for i in idx)] = blocks[order[slot]].reshape((4,) * dims)
    if partial:
        a = np.ascontiguousarray(a[tuple(slice(0, s - 1) for s in shape)])
    a.setflags(write=False)
    _cache[key] = a
    return a


def int_field(dims, dtype):
    """Integers spanning the documented lossy range on the ladder field's shape
    (one element cut off every axis), for the integer rates."""
    import layouts
    dtype = np.dtype(dtype)
    key = ("int", dims, dtype)
    if key not in _cache:
        shape = ladder_field(dims, F32, True).shape
        a = layouts.edge_ints(shape, dtype, np.random.default_rng(40 + dims), False)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]
