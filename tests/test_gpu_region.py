"""Region decode on the GPU (zfp_hip_decompress_region and the layers above it).

Expected values are the oracle's: oracle.decompress_words of the oracle's own
stream for the coded box, cropped with numpy -- never the product's full decode.
(Integer fields, which the oracle does not code, take both from the reference
library as test_gpu_types.py does.)  Every case decodes into a strided view
inside a larger sentinel-filled array with a guard band on every side and
asserts (i) the region's bytes, (ii) untouched guard bands, (iii) blocks_read ==
the number of blocks that intersect the region -- a decoder that falls back to
decoding everything fails (iii).
"""
import ctypes
import os
import zlib

import numpy as np
import pytest

from pyoracle import (TYPE_DOUBLE, TYPE_FLOAT, params_accuracy, params_precision, params_rate,
                      params_reversible)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_HIP = os.path.join(REPO, "zfp-par_amd", "lib", "libzfp_hip.so")
TYPES = {np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.float32): 3, np.dtype(np.float64): 4}
SENTINEL = 0xA5
GUARD = (1, 2, 4)  # elements on either side, slowest axis first (x: a multiple of 4, so 16-byte rows can occur)


class Job(ctypes.Structure):
    """zfp_hip_job (include/zfp_hip.h)."""
    _fields_ = [("type", ctypes.c_int32), ("dims", ctypes.c_int32), ("n", ctypes.c_uint64 * 4),
                ("s", ctypes.c_int64 * 4), ("f", ctypes.c_uint64 * 4), ("e", ctypes.c_uint64 * 4),
                ("minbits", ctypes.c_uint32), ("maxbits", ctypes.c_uint32), ("maxprec", ctypes.c_uint32),
                ("minexp", ctypes.c_int32)]


@pytest.fixture(scope="module")
def hip(product):
    lib = ctypes.CDLL(LIB_HIP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.zfp_hip_decompress_region.restype = ctypes.c_int
    lib.zfp_hip_decompress_region.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, ctypes.c_int, vp, vp]
    lib.zfp_hip_index_build.restype = ctypes.c_int
    lib.zfp_hip_index_build.argtypes = [vp, vp, u64, u64, ctypes.c_int, vp]
    lib.zfp_hip_index_create.restype = vp
    lib.zfp_hip_index_free.argtypes = [vp]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


def _params(mode, param, ztype, dims):
    if mode == "rate":
        return params_rate(param, ztype, dims)
    if mode == "precision":
        return params_precision(param)
    if mode == "accuracy":
        return params_accuracy(param)
    return params_reversible()


def _special_field(shape, dtype, rng):
    a = (rng.standard_normal(shape) * rng.choice([1e-3, 1.0, 1e5], size=shape)).astype(dtype)
    flat = a.reshape(-1)
    info = np.finfo(dtype)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, info.tiny, info.tiny / 4, -info.tiny / 8,
                         info.max, -info.max], dtype=dtype)
    idx = rng.choice(flat.size, size=max(1, flat.size // 40), replace=False)
    flat[idx] = rng.choice(specials, size=idx.size)
    if min(shape) >= 8:
        a[:4, :4, :4] = info.tiny / 16
        a[4:8, :4, :4] = -0.0
        a[:4, 4:8, :4] = 0.0
        a[4:8, 4:8, :4] = np.nan
    return a


def _job(shape, ztype, params, coded=None):
    """shape, coded: numpy axis order (slowest first); coded = [(f, e)] or None for the whole field."""
    dims = len(shape)
    j = Job()
    j.type, j.dims = ztype, dims
    for a in range(dims):
        j.n[a] = shape[dims - 1 - a]
        j.f[a], j.e[a] = coded[dims - 1 - a] if coded else (0, shape[dims - 1 - a])
    j.minbits, j.maxbits, j.maxprec, j.minexp = params
    return j


def _arr4(ctype, vals):
    vals = list(reversed(list(vals)))
    return (ctype * 4)(*(vals + [0] * (4 - len(vals))))


def _blocks(region, coded, shape):
    n = 1
    for (lo, hi), (f, _) in zip(region, coded or [(0, s) for s in shape]):
        n *= (hi - 1 - f) // 4 - (lo - f) // 4 + 1
    return n


def _guarded(ext, dtype):
    """(big, view): a sentinel-filled array and the strided view of extents `ext` inside its guard bands."""
    g = GUARD[3 - len(ext):]
    full = [n + 2 * k for n, k in zip(ext, g)]
    full[-1] = (full[-1] + 3) // 4 * 4
    big = np.empty(full, dtype=dtype)
    big.view(np.uint8)[...] = SENTINEL
    return big, big[tuple(slice(k, k + n) for n, k in zip(ext, g))]


def _region_decode(hip, job, region, view_ptr, view_strides, words_ptr, nwords, bit_offset=0, index=None):
    blocks = ctypes.c_uint64(0)
    rc = hip.zfp_hip_decompress_region(ctypes.byref(job), _arr4(ctypes.c_uint64, [lo for lo, _ in region]),
                                       _arr4(ctypes.c_uint64, [hi for _, hi in region]), view_ptr,
                                       _arr4(ctypes.c_int64, view_strides), words_ptr, nwords, bit_offset, -1, index,
                                       ctypes.byref(blocks))
    assert rc == 1, hip.zfp_hip_last_error().decode()
    return blocks.value


def _check(hip, words, shape, dtype, params, ref, region, coded=None, bit_offset=0, index=None, ztype=None):
    """One region of one stream into a guarded host view: (i) bytes, (ii) guards, (iii) blocks_read."""
    dtype = np.dtype(dtype)
    region = [(0 if r is None else r[0], n if r is None else r[1]) for r, n in zip(region, shape)]
    job = _job(shape, ztype or TYPES[dtype], params, coded)
    big, view = _guarded([hi - lo for lo, hi in region], dtype)
    got = _region_decode(hip, job, region, view.ctypes.data, [s // dtype.itemsize for s in view.strides],
                         words.ctypes.data, len(words), bit_offset, index)
    want = ref[tuple(slice(lo, hi) for lo, hi in region)]
    assert np.ascontiguousarray(view).tobytes() == np.ascontiguousarray(want).tobytes(), (region, "values")
    view.view(np.uint8)[...] = SENTINEL
    assert (big.view(np.uint8) == SENTINEL).all(), (region, "guard band written")
    assert got == _blocks(region, coded, shape), (region, "blocks_read")


# ---------------------------------------------------------------------------
MODES = [("rate", 16), ("rate", 8), ("rate", 5), ("rate", 3.25), ("precision", 20), ("accuracy", 1e-3),
         ("reversible", None)]
SHAPE = (21, 26, 72)  # 18 blocks along x, partial edge blocks on all three axes
REGIONS = [
    (None, None, None),                   # the whole field
    ((10, 11), (13, 14), (37, 38)),       # one element
    ((9, 11), (13, 15), (37, 39)),        # inside one block
    ((3, 19), (5, 22), (6, 70)),          # unaligned on both ends of every axis
    ((9, 10), None, None),                # one slice per axis, none at a multiple of 4
    (None, (13, 14), None),
    (None, None, (37, 38)),
    ((20, 21), (24, 26), (69, 72)),       # the last partial block's corner
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode,param", MODES)
def test_regions_match_oracle_all_modes(hip, oracle, dtype, mode, param):
    rng = np.random.default_rng(zlib.crc32(repr((mode, param, np.dtype(dtype).name)).encode()))
    a = _special_field(SHAPE, dtype, rng)
    params = _params(mode, param, TYPES[np.dtype(dtype)], 3)
    words, _ = oracle.compress_words(a, params)
    ref, _ = oracle.decompress_words(words, SHAPE, dtype, params)
    for region in REGIONS:
        _check(hip, words, SHAPE, dtype, params, ref, region)


@pytest.mark.parametrize("dtype,mode,param", [(np.float32, "rate", 12), (np.float64, "precision", 32)])
def test_long_rows_cross_waves_and_workgroups(hip, oracle, dtype, mode, param):
    """75 blocks per x-row: a wave's blocks span rows, more than one workgroup
    is in flight; f64 at precision 32 is the planes-32..63 decoder."""
    shape = (8, 8, 300)
    rng = np.random.default_rng(5)
    a = _special_field(shape, dtype, rng)
    params = _params(mode, param, TYPES[np.dtype(dtype)], 3)
    words, _ = oracle.compress_words(a, params)
    ref, _ = oracle.decompress_words(words, shape, dtype, params)
    for region in [((0, 8), (0, 8), (2, 299)), ((1, 6), (2, 7), (250, 300))]:
        _check(hip, words, shape, dtype, params, ref, region)


@pytest.mark.parametrize("mode,param", [("rate", 8), ("reversible", None)])
def test_stream_behind_a_header(hip, oracle, mode, param):
    """Blocks start at bit 96, as in a stream zfpy wrote."""
    rng = np.random.default_rng(11)
    shape = (20, 24, 36)
    a = rng.standard_normal(shape).astype(np.float32)
    params = _params(mode, param, 0, 3)
    words, _ = oracle.compress_words(a, params, bit_offset=96)
    ref, _ = oracle.decompress_words(words, shape, np.float32, params, bit_offset=96)
    for region in [((1, 18), (3, 23), (5, 34)), ((7, 8), None, (2, 35))]:
        _check(hip, words, shape, np.float32, params, ref, region, bit_offset=96)


@pytest.mark.parametrize("mode,param", [("rate", 8), ("precision", 20)])
def test_coded_chunk_inside_a_larger_field(hip, oracle, mode, param):
    shape = (24, 24, 48)
    coded = [(8, 20), (4, 24), (12, 40)]
    rng = np.random.default_rng(3)
    a = _special_field(shape, np.float32, rng)
    params = _params(mode, param, TYPE_FLOAT, 3)
    box = list(reversed(coded)) + [(0, 0)]
    words, _ = oracle.compress_words(a, params, box=box)
    ref, _ = oracle.decompress_words(words, shape, np.float32, params, box=box)
    for region in [((8, 13), (4, 11), (12, 30)),      # low corner at the box's f
                   ((10, 19), (9, 22), (17, 39)),     # interior
                   ((8, 20), (4, 24), (12, 40))]:     # the whole box
        _check(hip, words, shape, np.float32, params, ref, region, coded=coded)


def _export(lib, idx):
    n = lib.zfp_hip_index_export(idx, None, 0)
    blob = ctypes.create_string_buffer(n)
    assert lib.zfp_hip_index_export(idx, blob, n) == n
    return bytearray(blob.raw)


def test_index_handling(hip, product, oracle):
    """Variable rate: the encoder's index (no scan), no index (scan), an index of
    another stream of the same shape that passes the fingerprint (caught by the
    block lengths, rescanned), and one index object across regions and a rebuild."""
    lib = product.lib
    rng = np.random.default_rng(17)
    a = _special_field(SHAPE, np.float32, rng)
    b = _special_field(SHAPE, np.float32, rng)
    params = params_precision(20)
    wa, _ = oracle.compress_words(a, params)
    wb, _ = oracle.compress_words(b, params)
    ra, _ = oracle.decompress_words(wa, SHAPE, np.float32, params)
    rb, _ = oracle.decompress_words(wb, SHAPE, np.float32, params)
    unaligned = ((3, 19), (5, 22), (6, 70))
    whole = (None, None, None)
    # the encoder's index (the product's stream is the oracle's, bit for bit)
    assert product.compress(a, "precision", 20) == wa.tobytes()
    ia = product.last_index
    assert product.compress(b, "precision", 20) == wb.tobytes()
    ib = product.last_index
    product.last_index = None
    try:
        for region in (unaligned, whole):
            _check(hip, wa, SHAPE, np.float32, params, ra, region, index=ia)
            assert product.last_scan() is None and lib.zfp_hip_last_stale_index() == 0
        # no index
        _check(hip, wa, SHAPE, np.float32, params, ra, unaligned)
        assert product.last_scan() is not None and lib.zfp_hip_last_stale_index() == 0
        # b's lengths and bases under a's bit count and fingerprint
        ea, eb = _export(lib, ia), _export(lib, ib)
        eb[24:32] = ea[24:32]  # total bits
        eb[48:56] = ea[48:56]  # fingerprint
        wrong = lib.zfp_hip_index_import(bytes(eb), len(eb))
        assert wrong
        for region in (whole, unaligned):
            _check(hip, wa, SHAPE, np.float32, params, ra, region, index=wrong)
            assert lib.zfp_hip_last_stale_index() == 1 and product.last_scan() is not None
        lib.zfp_hip_index_free(wrong)
    finally:
        lib.zfp_hip_index_free(ia)
        lib.zfp_hip_index_free(ib)
    # one index object: two regions in a row (the cached start table is reused),
    # then rebuilt for another stream (the table must follow)
    job = _job(SHAPE, TYPE_FLOAT, params)
    idx = hip.zfp_hip_index_create()
    try:
        assert hip.zfp_hip_index_build(ctypes.byref(job), wa.ctypes.data, len(wa), 0, -1, idx) == 1
        for region in (unaligned, ((9, 10), None, None)):
            _check(hip, wa, SHAPE, np.float32, params, ra, region, index=idx)
            assert product.last_scan() is None and lib.zfp_hip_last_stale_index() == 0
        assert hip.zfp_hip_index_build(ctypes.byref(job), wb.ctypes.data, len(wb), 0, -1, idx) == 1
        _check(hip, wb, SHAPE, np.float32, params, rb, unaligned, index=idx)
        assert product.last_scan() is None and lib.zfp_hip_last_stale_index() == 0
    finally:
        hip.zfp_hip_index_free(idx)


def _int_field(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    idx = np.indices(shape, dtype=np.float64)
    smooth = sum(np.sin(0.07 * (k + 1) * idx[k]) for k in range(len(shape)))
    scale = 1 << (20 if np.dtype(dtype).itemsize == 4 else 40)
    return ((smooth * scale).astype(np.int64) + rng.integers(-999, 1000, size=shape)).astype(dtype)


@pytest.mark.parametrize("mode,param", [("rate", 8), ("reversible", None)])
@pytest.mark.parametrize("dtype,shape,region", [(np.float32, (13, 37), ((2, 11), (5, 34))),
                                                (np.float64, (70,), ((3, 66),))])
def test_1d_2d_floats_match_oracle(hip, oracle, dtype, shape, region, mode, param):
    rng = np.random.default_rng(29)
    a = (rng.standard_normal(shape) * 100).astype(dtype)
    params = _params(mode, param, TYPES[np.dtype(dtype)], len(shape))
    words, _ = oracle.compress_words(a, params)
    ref, _ = oracle.decompress_words(words, shape, dtype, params)
    for r in (region, (None,) * len(shape)):
        _check(hip, words, shape, dtype, params, ref, r)


@pytest.mark.parametrize("mode,param", [("rate", 8), ("reversible", None)])
@pytest.mark.parametrize("dtype,shape,region", [(np.int32, (70,), ((3, 66),)),
                                                (np.int64, (13, 37), ((2, 11), (5, 34)))])
def test_1d_2d_integers_match_reference(hip, ref_capi, dtype, shape, region, mode, param):
    """The oracle codes floats only: the stream and the expected values are the
    reference library's, as in test_gpu_types.py."""
    a = _int_field(shape, dtype, 31)
    ztype = TYPES[np.dtype(dtype)]
    data = ref_capi.compress(a, mode, param, ztype=ztype)
    ref, _ = ref_capi.decompress(data, shape, dtype, mode, param, ztype=ztype)
    words = np.frombuffer(data + bytes((-len(data)) % 8), dtype=np.uint64).copy()
    params = _params(mode, param, ztype, len(shape))
    for r in (region, (None,) * len(shape)):
        _check(hip, words, shape, dtype, params, ref, r)


@pytest.mark.parametrize("mode,param,region", [("rate", 8, ((10, 11), None, None)),
                                               ("precision", 20, ((3, 19), (5, 22), (6, 70)))])
def test_host_and_device_memory(hip, oracle, mode, param, region):
    """The four combinations of host or device stream and destination agree
    (the host fixed-rate stream case is the thin region [10:11, :, :], of which
    only the needed words are staged)."""
    import torch
    rng = np.random.default_rng(23)
    a = _special_field(SHAPE, np.float32, rng)
    params = _params(mode, param, TYPE_FLOAT, 3)
    words, _ = oracle.compress_words(a, params)
    ref, _ = oracle.decompress_words(words, SHAPE, np.float32, params)
    reg = [(0 if r is None else r[0], n if r is None else r[1]) for r, n in zip(region, SHAPE)]
    want = np.ascontiguousarray(ref[tuple(slice(lo, hi) for lo, hi in reg)])
    job = _job(SHAPE, TYPE_FLOAT, params)
    d_words = torch.from_numpy(words.view(np.int64).copy()).cuda()
    for dev_stream in (False, True):
        for dev_dst in (False, True):
            big, view = _guarded([hi - lo for lo, hi in reg], np.float32)
            strides = [s // 4 for s in view.strides]
            wptr = d_words.data_ptr() if dev_stream else words.ctypes.data
            if dev_dst:
                d_big = torch.from_numpy(big).cuda()
                ptr = d_big.data_ptr() + (view.ctypes.data - big.ctypes.data)
            else:
                ptr = view.ctypes.data
            got = _region_decode(hip, job, reg, ptr, strides, wptr, len(words))
            if dev_dst:
                torch.cuda.synchronize()
                big[...] = d_big.cpu().numpy()
            assert np.ascontiguousarray(view).tobytes() == want.tobytes(), (dev_stream, dev_dst)
            view.view(np.uint8)[...] = SENTINEL
            assert (big.view(np.uint8) == SENTINEL).all(), (dev_stream, dev_dst, "guard band written")
            assert got == _blocks(reg, None, SHAPE)


def _strided_views(ext, dtype):
    """[(name, big, view)]: views of extents `ext` inside sentinel-filled arrays
    whose x stride is 2, whose y axis is reversed, and both."""
    out = []
    for name, xs, yrev in (("x stride 2", 2, False), ("y reversed", 1, True), ("x stride 2, y reversed", 2, True)):
        g = GUARD[3 - len(ext):]
        big = np.empty([n + 2 * k for n, k in zip(ext[:-1], g)] + [xs * ext[-1] + 2 * g[-1]], dtype=dtype)
        big.view(np.uint8)[...] = SENTINEL
        view = big[tuple(slice(k, k + n) for n, k in zip(ext[:-1], g)) + (slice(g[-1], g[-1] + xs * ext[-1], xs),)]
        out.append((name, big, view[:, ::-1, :] if yrev else view))
    return out


@pytest.mark.parametrize("mode,param", [("rate", 8), ("precision", 20)])
def test_host_destination_with_x_stride_and_negative_y_stride(hip, oracle, mode, param):
    """A host destination whose rows are not contiguous or run backwards: the
    region's elements land where the strides say and nothing else is written."""
    shape = (9, 10, 13)  # partial blocks on every axis
    region = [(2, 7), (1, 9), (3, 12)]
    rng = np.random.default_rng(61)
    a = _special_field(shape, np.float32, rng)
    params = _params(mode, param, TYPE_FLOAT, 3)
    words, _ = oracle.compress_words(a, params)
    ref, _ = oracle.decompress_words(words, shape, np.float32, params)
    want = ref[tuple(slice(lo, hi) for lo, hi in region)]
    job = _job(shape, TYPE_FLOAT, params)
    for name, big, view in _strided_views([hi - lo for lo, hi in region], np.float32):
        got = _region_decode(hip, job, region, view.ctypes.data, [s // 4 for s in view.strides], words.ctypes.data,
                             len(words))
        assert np.ascontiguousarray(view).tobytes() == np.ascontiguousarray(want).tobytes(), (name, "values")
        view[...] = np.frombuffer(bytes([SENTINEL] * 4), dtype=np.float32)[0]  # (an ordinary value: stored as it is)
        assert (big.view(np.uint8) == SENTINEL).all(), (name, "bytes outside the region written")
        assert got == _blocks(region, None, shape), (name, "blocks_read")


def test_4d_is_refused(hip):
    shape = (8, 8, 8, 8)
    job = _job(shape, TYPE_FLOAT, params_rate(8, TYPE_FLOAT, 4))
    out = np.full(4096, SENTINEL, dtype=np.uint8)
    words = np.zeros(4096, dtype=np.uint64)
    rc = hip.zfp_hip_decompress_region(ctypes.byref(job), _arr4(ctypes.c_uint64, (0, 0, 0, 0)),
                                       _arr4(ctypes.c_uint64, (4, 4, 4, 4)), out.ctypes.data,
                                       _arr4(ctypes.c_int64, (64, 16, 4, 1)), words.ctypes.data, len(words), 0, -1, None,
                                       None)
    assert rc == 0
    assert "4D" in hip.zfp_hip_last_error().decode()
    assert (out == SENTINEL).all()


# ---------------------------------------------------------------------------
def test_zfpy_decompress_region():
    import zfpy
    rng = np.random.default_rng(41)
    a = rng.standard_normal(SHAPE).astype(np.float32)
    region = (slice(3, 19), slice(5, 22), slice(6, 70))
    s = zfpy.compress_numpy(a, rate=8)
    got = zfpy.decompress_region(s, region)
    assert got.flags.c_contiguous and got.shape == (16, 17, 64)
    assert got.tobytes() == np.ascontiguousarray(zfpy.decompress_numpy(s)[region]).tobytes()
    s = zfpy.compress_numpy(a, precision=20)
    assert getattr(s, "block_index", None) is not None
    want = np.ascontiguousarray(zfpy.decompress_numpy(s)[region]).tobytes()
    assert zfpy.decompress_region(s, region).tobytes() == want
    assert zfpy.decompress_region(bytes(s), region).tobytes() == want  # the index is dropped: scanned
    assert zfpy.decompress_region(s, (None, slice(None), slice(70, 72))).tobytes() == \
        np.ascontiguousarray(zfpy.decompress_numpy(s)[:, :, 70:72]).tobytes()


@pytest.mark.parametrize("mode", [dict(rate=8), dict(precision=16)])
def test_zfp_parallel_decompress_region(mode):
    import zfpy
    shape = (64, 64, 96)
    rng = np.random.default_rng(43)
    idx = np.indices(shape, dtype=np.float32)
    a = (np.sin(0.05 * idx[0]) + np.cos(0.07 * idx[1]) * np.sin(0.03 * idx[2])
         + 1e-3 * rng.standard_normal(shape)).astype(np.float32)
    zp = zfpy.zfp_parallel(shape, "float32", nparts=8)
    zp.get_numpy_array()[...] = a
    zp.compress(nthreads=8, **mode)
    boxes = zp.get_chunkit().boxes
    assert len(boxes) == 8
    zp.get_numpy_array()[...] = 7.0
    straddle = (slice(5, 61), slice(3, 62), slice(7, 90))
    x, y, z = boxes[3][:3]  # one chunk's box (x first)
    inside = (slice(z[0] + 1, z[1] - 1), slice(y[0] + 2, y[1] - 1), slice(x[0] + 3, x[1] - 2))
    parts = {name: zp.decompress_region(r, nthreads=8) for name, r in (("straddle", straddle), ("inside", inside))}
    assert (zp.get_numpy_array() == 7.0).all(), "decompress_region touched the shared array"
    zp.decompress(nthreads=8)
    full = np.array(zp.get_numpy_array())
    # the region straddles all eight chunks
    lo = [s.start for s in reversed(straddle)]
    hi = [s.stop for s in reversed(straddle)]
    assert all(all(lo[k] < b[k][1] and b[k][0] < hi[k] for k in range(3)) for b in boxes)
    for name, r in (("straddle", straddle), ("inside", inside)):
        assert parts[name].tobytes() == np.ascontiguousarray(full[r]).tobytes(), name
