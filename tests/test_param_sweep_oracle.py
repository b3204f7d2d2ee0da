"""The CPU oracle against the reference library over the whole parameter sweep
(tests/params.py): every rate, precision, tolerance and expert tuple, float32
and float64, 1D-4D, on the exponent-ladder field.  Stream bytes and decoded
bits (as unsigned integers) are the reference's.  The GPU sweep
(test_gpu_param_sweep.py) takes the oracle as the truth at these points.

Also: the sweep is not vacuous -- the tolerance list reaches both clamps of the
block precision and the rate list has truncated and padded blocks.
"""
import math

import numpy as np
import pytest

import layouts
import params as P
from pyoracle import (TYPE_DOUBLE, TYPE_FLOAT, ZFP_MAX_BITS, ZFP_MIN_EXP, have_ref, params_accuracy,
                      params_precision, params_rate)

pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built (make -C oracle ref)")

DTYPES = ["float32", "float64"]
AXES = ["rate", "precision", "accuracy", "expert"]


def ztype_of(dtype):
    return TYPE_FLOAT if np.dtype(dtype) == np.float32 else TYPE_DOUBLE


def param_list(axis, dtype):
    dtype = np.dtype(dtype)
    return {"rate": P.RATES, "precision": P.PRECISIONS, "accuracy": P.TOLERANCES, "expert": P.EXPERT}[axis][dtype]


def codec_params(axis, param, dtype, dims):
    if axis == "rate":
        return params_rate(param, ztype_of(dtype), dims)
    if axis == "precision":
        return params_precision(param)
    if axis == "accuracy":
        return params_accuracy(param)
    return tuple(param)


def test_lists_are_what_the_sweep_promises(ref_capi):
    for dtype in (P.F32, P.F64):
        h, hr = P.HEADER_BITS[dtype], P.HEADER_BITS_REVERSIBLE[dtype]
        assert len(P.EXPERT[dtype]) >= 40
        zs = ref_capi.zfp_stream_open(None)
        for t in P.EXPERT[dtype]:
            assert ref_capi.zfp_stream_set_params(zs, *t) == 1, t
            assert t[1] >= (hr if t[3] < ZFP_MIN_EXP else h), t
        ref_capi.zfp_stream_close(zs)
        for dims in (1, 2, 3, 4):
            for r in P.RATES[dtype]:
                assert h <= params_rate(r, ztype_of(dtype), dims)[1], (dims, r)
        assert set(range(1, 33)) <= set(P.PRECISIONS[dtype])
        assert 0.0 in P.TOLERANCES[dtype] and len(P.TOLERANCES[dtype]) == 24
        for tol in P.TOLERANCES[dtype]:
            assert params_accuracy(tol)[3] >= ZFP_MIN_EXP
    assert 80 in P.RATES[P.F32] and 64 in P.RATES[P.F64] and 16.01 in P.RATES[P.F32]


@pytest.mark.parametrize("dims", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ladder_field_shape_and_content(dims, dtype):
    a = P.ladder_field(dims, dtype, False)
    assert all(s % 4 == 0 for s in a.shape)
    nblocks = a.size // 4 ** dims
    assert 64 < nblocks < 1000 and nblocks % 64 != 0
    b = P.ladder_field(dims, dtype, True)
    assert b.shape == tuple(s - 1 for s in a.shape)
    # every exponent of the list is some block's largest magnitude, exactly
    blocks = a.reshape(sum(((s // 4, 4) for s in a.shape), ()))
    blocks = blocks.transpose(tuple(range(0, 2 * dims, 2)) + tuple(range(1, 2 * dims, 2))).reshape(nblocks, -1)
    with np.errstate(invalid="ignore"):
        top = np.abs(blocks.astype(np.float64)).max(axis=1)
    finite = top[np.isfinite(top) & (top > 0)]
    m, e = np.frexp(finite)
    pure = set((e[m == 0.5] - 1).tolist())
    assert set(P.ladder_exponents(dtype)) <= pure
    assert np.isnan(blocks).all(axis=1).any() and np.isinf(blocks).any()
    assert (blocks == 0).all(axis=1).sum() >= 2 and np.signbit(blocks).all(axis=1).any()


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("dims", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_matches_reference_over_the_sweep(oracle, ref_capi, dtype, dims, axis):
    a = P.ladder_field(dims, dtype, True)
    u = layouts.uint_of(a.dtype)
    bad, ran = [], 0
    plist = param_list(axis, dtype)
    for param in plist:
        cp = codec_params(axis, param, dtype, dims)
        ref = ref_capi.compress(a, axis, param, ztype=ztype_of(dtype))
        words, end = oracle.compress_words(a, cp)
        mine = words.view(np.uint8).tobytes()
        ref_out, n = ref_capi.decompress(ref, a.shape, a.dtype, axis, param, ztype=ztype_of(dtype))
        out, end2 = oracle.decompress_words(words, a.shape, a.dtype, cp)
        # (encode and decode ends are compared with the reference's, not with each other: the
        # reference's reversible encoder writes a zero block as one bit without padding it to
        # minbits, and its decoder skips minbits there)
        ok = (end + 63) // 64 * 8 == len(ref) and mine == ref and (end2 + 63) // 64 * 8 == n and \
            out.view(u).tobytes() == ref_out.view(u).tobytes()
        if not ok:
            bad.append(param)
        ran += 1
    assert not bad, bad
    assert ran == len(plist)


def _block_top_exponents(a, dims):
    """The codec's exponent of each whole block's largest magnitude: frexp's, not
    below that of the smallest normal number (None: zero or not finite)."""
    nb = [s // 4 for s in a.shape]
    floor = np.finfo(a.dtype).minexp + 1
    out = []
    for idx in np.ndindex(*nb):
        blk = a[tuple(slice(4 * i, 4 * i + 4) for i in idx)].astype(np.float64)
        top = np.abs(blk).max()
        out.append(max(math.frexp(top)[1], floor) if np.isfinite(top) and top > 0 else None)
    return out


@pytest.mark.parametrize("dims", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tolerances_reach_both_precision_clamps(oracle, dtype, dims):
    """Some block is header-only (precision 0: one bit) and some block is coded at
    maxprec (emax - minexp + 2 (dims + 1) >= maxprec) over the tolerance list."""
    a = P.ladder_field(dims, dtype, False)
    emax = _block_top_exponents(a, dims)
    header_only = at_maxprec = 0
    for tol in P.TOLERANCES[np.dtype(dtype)]:
        cp = params_accuracy(tol)
        lens = oracle.block_bits(a, cp)
        assert len(lens) == len(emax)
        for n, e in zip(lens.tolist(), emax):
            if e is None:
                continue
            prec = e - cp[3] + 2 * (dims + 1)
            if prec <= 0:
                assert n == 1, (tol, e, n)
                header_only += 1
            elif prec >= cp[2]:
                assert n > 1
                at_maxprec += 1
    assert header_only > 0 and at_maxprec > 0


@pytest.mark.parametrize("dims", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rates_truncate_and_pad(oracle, dtype, dims):
    """Over the rate list some block outruns its budget and some block is padded."""
    a = P.ladder_field(dims, dtype, False)
    free = oracle.block_bits(a, (1, ZFP_MAX_BITS, 64, ZFP_MIN_EXP))  # what each block codes without a budget
    truncated = padded = 0
    for rate in P.RATES[np.dtype(dtype)]:
        cp = params_rate(rate, ztype_of(dtype), dims)
        lens = oracle.block_bits(a, cp)
        assert (lens == cp[1]).all(), rate
        truncated += int((free > cp[1]).sum())
        padded += int((free < cp[1]).sum())
    assert truncated > 0 and padded > 0
    if np.dtype(dtype) == np.float32:
        # the budget exceeds every float block (3D: 9 + 63 + 2048 = 2120 bits, rate 34 and up): nothing reaches it
        for rate in (34, 80) if dims == 3 else (80,):
            assert (free < params_rate(rate, TYPE_FLOAT, dims)[1]).all()
