"""The codec parameters themselves, swept on the GPU (tests/params.py): every
rate, precision, tolerance and expert tuple of the lists, float32 and float64
in 1D-4D against the oracle (pinned to the reference at these very points by
test_param_sweep_oracle.py), integer fields at the integer rates against the
reference library, all through the C API.

  compressed bytes and length equal the truth's;
  zfp_decompress of the truth's bytes gives the truth's decode, bit for bit,
  and returns the size the truth's decode consumed (variable rate: once with
  the encoder's index, once with the scan).

Fields are the exponent ladder with one element cut off every axis.  The 3D
rates also run on a device-resident 64x16x16 field into a device stream (one
whole workgroup: even word counts take encode3_aligned_full, odd ones and a
stream start that is not 16-byte aligned encode3_aligned, a block that does not
fit the aligned slots the general kernel), and 1D-3D integer rates decode and
rewrite one off-origin region.

Each test loops over its list, collects every failing parameter and asserts at
the end, so one run shows the whole picture; nothing is skipped, and the number
of cases run must equal the length of the list.
"""
import ctypes

import numpy as np
import pytest

import layouts
import params as P
import test_gpu_region as tr
import test_gpu_region_encode as tre
from test_gpu_encode_slots import _dev_compress
from test_param_sweep_oracle import AXES, codec_params, param_list, ztype_of

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
_dev_truth = {}  # the device-field streams, shared by the two stream starts


def truth(oracle, a, cp):
    """(stream bytes, decode, bytes the decode consumed) of the oracle."""
    words, end = oracle.compress_words(a, cp)
    out, dend = oracle.decompress_words(words, a.shape, a.dtype, cp)
    return words.view(np.uint8).tobytes()[: (end + 63) // 64 * 8], out, (dend + 63) // 64 * 8


def _free_index(product):
    if product.last_index:
        product.lib.zfp_hip_index_free(product.last_index)
    product.last_index = None


def _sweep_one(product, a, mode, param, ztype, want, ref_out, want_n, fixed):
    """One parameter through zfp_compress and zfp_decompress: a list of what differs."""
    u = layouts.uint_of(a.dtype)
    bad = []
    product.last_index = None
    got = product.compress(a, mode, param, ztype=ztype)
    index = product.last_index
    try:
        if len(got) != len(want):
            bad.append("compressed length %d, truth %d (%s)" % (len(got), len(want), product.lib.zfp_hip_last_error()))
        elif got != want:
            bad.append("compressed bytes differ")
        if not fixed and not index:
            bad.append("no block index from a variable-rate encode")
        # The stream as the truth's decoder consumed it.  One tuple of the lists decodes past the end of
        # what its encoder wrote (reversible with minbits 300: the reference's encoder writes a zero block
        # as one bit, its decoder skips minbits there) and so reads zeros the caller's buffer happens to
        # hold; the product is given those bytes too.  Short of them it must refuse the stream, not read on.
        stream = want + bytes(max(0, want_n - len(want)))
        if len(stream) > len(want):
            out, n = product.decompress(want, a.shape, a.dtype, mode, param, ztype=ztype)
            if n != 0 or b"stream holds" not in product.lib.zfp_hip_last_error():
                bad.append("a stream that ends before its last block: returned %d (%s)" %
                           (n, product.lib.zfp_hip_last_error()))
        for idx in ((None,) if fixed else (index, None)):  # the encoder's index, then the scan
            if not fixed and idx is None and index is None:
                continue
            out, n = product.decompress(stream, a.shape, a.dtype, mode, param, ztype=ztype, index=idx)
            how = "scan" if idx is None and not fixed else "index" if idx else "fixed"
            if n != want_n:
                bad.append("decompress (%s) returned %d, truth %d (%s)" % (how, n, want_n,
                                                                            product.lib.zfp_hip_last_error()))
            elif out.view(u).tobytes() != ref_out.view(u).tobytes():
                bad.append("decoded bits differ (%s)" % how)
    finally:
        _free_index(product)
    return bad


def _is_fixed(cp, h):
    return cp[0] == cp[1] and cp[3] >= P.ZFP_MIN_EXP and cp[1] >= h


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("dims", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_float_sweep_matches_oracle(product, oracle, dtype, dims, axis):
    a = P.ladder_field(dims, dtype, True)
    plist = param_list(axis, dtype)
    failures, ran = {}, 0
    for param in plist:
        cp = codec_params(axis, param, dtype, dims)
        want, ref_out, want_n = truth(oracle, a, cp)
        bad = _sweep_one(product, a, axis, param, ztype_of(dtype), want, ref_out, want_n,
                         _is_fixed(cp, P.HEADER_BITS[np.dtype(dtype)]))
        if bad:
            failures[str(param)] = bad
        ran += 1
    assert not failures, failures
    assert ran == len(plist)


@pytest.mark.parametrize("dims", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_integer_rates_match_reference(product, ref_capi, dtype, dims):
    a = P.int_field(dims, dtype)
    plist = P.INT_RATES[np.dtype(dtype)]
    failures, ran = {}, 0
    for rate in plist:
        want = ref_capi.compress(a, "rate", rate)
        ref_out, want_n = ref_capi.decompress(want, a.shape, a.dtype, "rate", rate)
        bad = _sweep_one(product, a, "rate", rate, None, want, ref_out, want_n, True)
        if bad:
            failures[str(rate)] = bad
        ran += 1
    assert not failures, failures
    assert ran == len(plist)


@pytest.mark.parametrize("start", [0, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rates_3d_device_field_whole_workgroup(product, oracle, dtype, start):
    """64x16x16, 256 blocks, field and stream device resident; `start`: the byte
    offset of the stream in its (16-byte aligned) buffer."""
    dims = (64, 16, 16)
    a = P.ladder_field(3, dtype, False, grid=(16, 4, 4))
    assert a.shape == (16, 16, 64)
    plist = P.RATES[np.dtype(dtype)]
    failures, ran = {}, 0
    for rate in plist:
        cp = codec_params("rate", rate, dtype, 3)
        if (dtype, cp) not in _dev_truth:
            _dev_truth[dtype, cp] = truth(oracle, a, cp)[0]
        want = _dev_truth[dtype, cp]
        got, = _dev_compress(product, a, dims, rate, start=start)
        if got != want:
            failures[str(rate)] = "length %d, truth %d" % (len(got), len(want)) if len(got) != len(want) else "bytes differ"
        ran += 1
    assert not failures, failures
    assert ran == len(plist)


# ---------------------------------------------------------------------------
# Regions at every integer rate.  The region kernels stage one block per lane in
# LDS: W = ceil(maxbits / 64) + 1 words at an odd stride for 256 lanes, beside
# their tables (2 KB decode, 4 KB encode) and 2 KB of lane state, in 160 KB:
# 2048 (W | 1) + 6 KB <= 160 KB, W | 1 <= 77, maxbits <= 4864.  A longer block is
# refused before anything is queued.
REGION_MAXBITS = 4864


@pytest.fixture(scope="module")
def hip(product):
    lib = ctypes.CDLL(tr.LIB_HIP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.zfp_hip_decompress_region.restype = ctypes.c_int
    lib.zfp_hip_decompress_region.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, ctypes.c_int, vp, vp]
    lib.zfp_hip_compress_region.restype = ctypes.c_int
    lib.zfp_hip_compress_region.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, ctypes.c_int, vp]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


def _refused(hip, job, region, a, words, maxbits):
    """Both region calls refuse a block that does not fit their staging: return
    value 0, the error text, destination and stream untouched."""
    bad = []
    text = "block size too large for LDS staging (%d bits)" % maxbits
    lo = tr._arr4(ctypes.c_uint64, [r[0] for r in region])
    hi = tr._arr4(ctypes.c_uint64, [r[1] for r in region])
    big, view = tr._guarded([r[1] - r[0] for r in region], a.dtype)
    strides = tr._arr4(ctypes.c_int64, [s // a.itemsize for s in view.strides])
    blocks = ctypes.c_uint64(0)
    rc = hip.zfp_hip_decompress_region(ctypes.byref(job), lo, hi, view.ctypes.data, strides, words.ctypes.data,
                                       len(words), 0, -1, None, ctypes.byref(blocks))
    if rc != 0 or text not in hip.zfp_hip_last_error().decode():
        bad.append("region decode: rc %d, %r" % (rc, hip.zfp_hip_last_error().decode()))
    if not (big.view(np.uint8) == tr.SENTINEL).all():
        bad.append("region decode refused but wrote its destination")
    stream = words.copy()
    src = np.ascontiguousarray(a[tuple(slice(l, h) for l, h in region)])
    rc = hip.zfp_hip_compress_region(ctypes.byref(job), lo, hi, src.ctypes.data,
                                     tr._arr4(ctypes.c_int64, [s // a.itemsize for s in src.strides]),
                                     stream.ctypes.data, len(stream), 0, -1, ctypes.byref(blocks))
    if rc != 0 or text not in hip.zfp_hip_last_error().decode():
        bad.append("region encode: rc %d, %r" % (rc, hip.zfp_hip_last_error().decode()))
    if stream.tobytes() != words.tobytes():
        bad.append("region encode refused but changed the stream")
    return bad


@pytest.mark.parametrize("dims", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_region_decode_and_rewrite_at_every_integer_rate(hip, oracle, dtype, dims):
    a = P.ladder_field(dims, dtype, True)
    # the rewrite's source: the same ladder, mirrored and negated
    new = np.ascontiguousarray(-a[tuple(slice(None, None, -1) for _ in a.shape)])
    region = tuple((1 + k, n - 2 - k) for k, n in enumerate(a.shape))  # off block origins on both ends
    plist = [r for r in P.RATES[np.dtype(dtype)] if r == int(r)]
    failures, ran, refused = {}, 0, 0
    for rate in plist:
        cp = codec_params("rate", rate, dtype, dims)
        codec = tre._Codec(oracle, a.shape, dtype, cp)
        words = codec.compress(a)
        try:
            if cp[1] > REGION_MAXBITS:
                refused += 1
                bad = _refused(hip, tr._job(a.shape, tr.TYPES[a.dtype], cp), region, a, words, cp[1])
                assert not bad, bad
            else:
                tr._check(hip, words, a.shape, dtype, cp, codec.decompress(words), region)
                tre._check(hip, codec, words, region, new, seed=int(rate))
        except AssertionError as e:
            failures[str(rate)] = str(e)[:300]
        ran += 1
    assert not failures, failures
    assert ran == len(plist)
    # float rate 80 in 3D is the list's one block past the staging (5120 bits)
    assert refused == (1 if (dtype, dims) == ("float32", 3) else 0)
