"""1D/2D fields of every scalar type and 3D/4D integer fields on the GPU.

The generic per-lane codec (blockn.h: encode_block_n / decode_block_n, the
closed-form coder with 4^d coefficients) and the integer branch of the 4D quad
codec (block4.h) against the reference library itself
(oracle/_ref, compiled from /root/reference): compressed bytes and
decompressed arrays identical, through the C API exactly as the reference's
end-to-end tests call it (tests/src/endtoend/zfpEndtoendBase.c).
"""
import zlib

import numpy as np
import pytest

import layouts
from pyoracle import params_accuracy, params_precision, params_rate, params_reversible
from test_gpu_codec import MODES as CODEC_MODES

pytestmark = pytest.mark.gpu

TYPES = {np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.float32): 3, np.dtype(np.float64): 4}


def _field(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    idx = np.indices(shape, dtype=np.float64)
    smooth = sum(np.sin(0.07 * (a + 1) * idx[a]) for a in range(len(shape)))
    if np.dtype(dtype).kind == "i":
        # integers well inside the range the reference transform is lossless for
        scale = 1 << (20 if np.dtype(dtype).itemsize == 4 else 40)
        a = (smooth * scale).astype(np.int64) + rng.integers(-999, 1000, size=shape)
        return a.astype(dtype)
    a = (smooth + 1e-2 * rng.standard_normal(shape)).astype(dtype)
    flat = a.reshape(-1)
    flat[rng.choice(flat.size, size=max(1, flat.size // 50), replace=False)] = 0  # zero runs, partial zero blocks
    if flat.size > 64:
        flat[:16] = 0  # an all-zero block
    return a


def _modes(dtype):
    if np.dtype(dtype).kind == "i":
        return [("rate", 8), ("rate", 20), ("rate", 32.5), ("precision", 12), ("precision", 30), ("reversible", None)]
    return [("rate", 8), ("rate", 16), ("precision", 18), ("accuracy", 1e-3), ("reversible", None)]


CASES = []
for dtype in (np.float32, np.float64, np.int32, np.int64):
    shapes = [(1000,), (37,), (45, 67), (64, 64)]
    if np.dtype(dtype).kind == "i":
        shapes += [(20, 24, 28), (9, 13, 7), (12, 9, 10, 11), (8, 16, 16, 16)]
    for shape in shapes:
        for mode, param in _modes(dtype):
            CASES.append((np.dtype(dtype).name, shape, mode, param))


@pytest.mark.parametrize("dtype,shape,mode,param", CASES)
def test_stream_and_roundtrip_match_reference(product, ref_capi, dtype, shape, mode, param):
    dtype = np.dtype(dtype)
    a = _field(shape, dtype, zlib.crc32(repr((dtype.name, shape, mode)).encode()))
    ztype = TYPES[dtype]
    want = ref_capi.compress(a, mode, param, ztype=ztype)
    product.keep_index = True
    try:
        got = product.compress(a, mode, param, ztype=ztype)
        assert got == want, (dtype.name, shape, mode, param)
        ref_out, _ = ref_capi.decompress(want, shape, dtype, mode, param, ztype=ztype)
        for index in (product.last_index, None):  # the encoder's index, then the scan
            out, n = product.decompress(got, shape, dtype, mode, param, ztype=ztype, index=index)
            assert n == len(got)
            assert out.tobytes() == ref_out.tobytes(), (dtype.name, shape, mode, param, index is None)
    finally:
        if product.last_index:
            product.lib.zfp_hip_index_free(product.last_index)
            product.last_index = None


@pytest.mark.parametrize("dtype", ["float32", "int32", "int64"])
def test_header_offset_2d(product, ref_capi, dtype):
    """zfpy layout (96-bit header first): unaligned block starts in 2D."""
    a = _field((33, 50), np.dtype(dtype), 5)
    ztype = 0 if dtype == "float32" else TYPES[np.dtype(dtype)]
    for mode, param in (("rate", 12), ("precision", 14), ("reversible", None)):
        want = ref_capi.compress(a, mode, param, ztype=ztype, header=True)
        got = product.compress(a, mode, param, ztype=ztype, header=True)
        assert got == want, (dtype, mode)
        ref_out, _ = ref_capi.decompress(want, a.shape, a.dtype, mode, param, ztype=ztype, header=True)
        out, _ = product.decompress(got, a.shape, a.dtype, mode, param, ztype=ztype, header=True)
        assert out.tobytes() == ref_out.tobytes(), (dtype, mode)


@pytest.mark.parametrize("shape,dtype", [((10000,), "float32"), ((90, 70), "float64"), ((50, 60), "int32")])
def test_threaded_chunks_sharing_pages(product, ref_capi, shape, dtype):
    """zfp_parallel decompresses the chunks of one array from a thread pool; chunk
    boundaries in 1D/2D fall inside memory pages, and every byte must still be
    the reference's (the library copies partial pages to the user array itself)."""
    import zfpy
    a = _field(shape, np.dtype(dtype), 9)
    zp = zfpy.zfp_parallel(shape, dtype, nparts=8)
    zp.get_numpy_array()[...] = a
    streams = zp.compress(nthreads=8, precision=20)
    whole = ref_capi.compress(a, "precision", 20, ztype=TYPES[np.dtype(dtype)])
    want, _ = ref_capi.decompress(whole, shape, dtype, "precision", 20, ztype=TYPES[np.dtype(dtype)])
    for _ in range(3):
        zp.get_numpy_array()[...] = 0
        zp._compress_data = [bytes(s) for s in streams]
        zp.decompress(nthreads=8)
        assert np.ascontiguousarray(zp.get_numpy_array()).tobytes() == want.tobytes()


# ---------------------------------------------------------------------------
# The generic per-lane codec on hard values: special floats in every mode and
# at odd stream offsets, integers at the edge of their range.
def _float_params(mode, param, ztype, dims):
    if mode == "rate":
        return params_rate(param, ztype, dims)
    if mode == "precision":
        return params_precision(param)
    if mode == "accuracy":
        return params_accuracy(param)
    return param if mode == "expert" else params_reversible()


# test_gpu_codec.MODES (its expert tuple pads short blocks to minbits) and an
# expert tuple whose small maxbits truncates blocks
HARD_MODES = CODEC_MODES + [("expert", (1, 40, 64, -1074))]
_HARD = {}


def _hard_field(dims, dtype):
    """NaN, +-Inf, +-0, denormals, +-max, 1e-3..1e5 and whole blocks of denormal,
    -0, 0 and NaN (layouts.special_field), one field per (dims, dtype)."""
    key = (dims, np.dtype(dtype).name)
    if key not in _HARD:
        a = layouts.special_field(layouts.SHAPES[dims], np.dtype(dtype), np.random.default_rng(zlib.crc32(repr(key).encode())))
        a.setflags(write=False)
        _HARD[key] = a
    return _HARD[key]


@pytest.mark.parametrize("mode,param", HARD_MODES)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("dims", [1, 2])
def test_special_values_1d_2d_match_oracle(product, oracle, dims, dtype, mode, param):
    a = _hard_field(dims, dtype)
    ztype = TYPES[a.dtype]
    params = _float_params(mode, param, ztype, dims)
    words, end = oracle.compress_words(a, params)
    want = words.view(np.uint8)[: (end + 63) // 64 * 8].tobytes()
    ref_out, _ = oracle.decompress_words(words, a.shape, a.dtype, params)
    product.last_index = None
    got = product.compress(a, mode, param, ztype=ztype)
    index = product.last_index
    try:
        assert got == want
        for idx in ((index, None) if index else (None,)):  # the encoder's index, then the scan
            out, n = product.decompress(want, a.shape, a.dtype, mode, param, ztype=ztype, index=idx)
            assert n == len(want), (idx is None, product.lib.zfp_hip_last_error())
            assert out.view(layouts.uint_of(a.dtype)).tobytes() == ref_out.view(layouts.uint_of(a.dtype)).tobytes(), \
                (idx is None)
    finally:
        if index:
            product.lib.zfp_hip_index_free(index)
        product.last_index = None


@pytest.mark.parametrize("mode,param", [("rate", 8), ("precision", 18)])
@pytest.mark.parametrize("pad", [1, 63, 100])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("dims", [1, 2])
def test_special_values_1d_2d_at_bit_offsets(product, oracle, dims, dtype, pad, mode, param):
    """Blocks that start at stream bit 1, 63 and 100 (stream_pad before the encode,
    stream_skip before the decode) against the oracle at the same bit offset."""
    a = _hard_field(dims, dtype)
    ztype = TYPES[a.dtype]
    params = _float_params(mode, param, ztype, dims)
    words, end = oracle.compress_words(a, params, bit_offset=pad)
    want = words.view(np.uint8)[: (end + 63) // 64 * 8].tobytes()
    ref_out, _ = oracle.decompress_words(words, a.shape, a.dtype, params, bit_offset=pad)
    product.last_index = None
    got = product.compress(a, mode, param, ztype=ztype, pad_bits=pad)
    index = product.last_index
    try:
        assert got == want
        for idx in ((index, None) if index else (None,)):
            out, n = product.decompress(want, a.shape, a.dtype, mode, param, ztype=ztype, index=idx, pad_bits=pad)
            assert n == len(want), (idx is None, product.lib.zfp_hip_last_error())
            assert out.view(layouts.uint_of(a.dtype)).tobytes() == ref_out.view(layouts.uint_of(a.dtype)).tobytes(), \
                (idx is None)
    finally:
        if index:
            product.lib.zfp_hip_index_free(index)
        product.last_index = None


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("dims", [1, 2, 3, 4])
def test_full_range_integers_reversible(product, ref_capi, dims, dtype):
    """Reversible mode on integers over the whole range of the type, with MIN,
    MAX, -1 and 0: the round trip returns the input exactly (the truth is the
    input; the transform's differences wrap) and the stream is the reference's
    (which round-trips these fields too: checked on the CPU)."""
    dtype = np.dtype(dtype)
    a = layouts.edge_ints(layouts.SHAPES[dims], dtype, np.random.default_rng(dims), True)
    info = np.iinfo(dtype)
    assert {info.min, info.max, -1, 0} <= set(a.reshape(-1).tolist())
    want = ref_capi.compress(a, "reversible", None)
    product.last_index = None
    got = product.compress(a, "reversible", None)
    index = product.last_index
    try:
        for idx in (index, None):
            out, n = product.decompress(got, a.shape, dtype, "reversible", None, index=idx)
            assert n == len(got)
            assert np.array_equal(out, a), (idx is None, "the round trip is not lossless")
        assert got == want
    finally:
        if index:
            product.lib.zfp_hip_index_free(index)
        product.last_index = None


@pytest.mark.parametrize("mode,param", [m for m in _modes(np.int32) if m[0] != "reversible"])
@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("dims", [1, 2, 3, 4])
def test_wide_integers_lossy_match_reference(product, ref_capi, dims, dtype, mode, param):
    """Rate and precision modes on integers spanning the documented lossy range,
    |x| < 2^30 (int32) and < 2^62 (int64): the high bit planes are in use."""
    dtype = np.dtype(dtype)
    a = layouts.edge_ints(layouts.SHAPES[dims], dtype, np.random.default_rng(10 + dims), False)
    lim = 1 << (np.iinfo(dtype).bits - 2)
    assert np.abs(a).max() == lim - 1
    want = ref_capi.compress(a, mode, param)
    ref_out, _ = ref_capi.decompress(want, a.shape, dtype, mode, param)
    product.last_index = None
    got = product.compress(a, mode, param)
    index = product.last_index
    try:
        assert got == want
        for idx in ((index, None) if index else (None,)):
            out, n = product.decompress(want, a.shape, dtype, mode, param, index=idx)
            assert n == len(want)
            assert out.tobytes() == ref_out.tobytes(), (idx is None)
    finally:
        if index:
            product.lib.zfp_hip_index_free(index)
        product.last_index = None
