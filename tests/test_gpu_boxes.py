"""Batched region decode on the GPU (zfp_hip_decompress_regions and the layers above it).

Expected values are the oracle's, as in test_gpu_region.py: oracle.decompress_words
of the oracle's own stream for the coded box, cropped with numpy (the int32 case
takes both from the reference library as test_gpu_types.py does).  Every
destination is a strided view inside a sentinel-filled array with guard bands;
every case asserts (i) each region's bytes, (ii) untouched guards, (iii)
blocks_read == the sum over the regions of the blocks that intersect each.
"""
import ctypes
import zlib

import numpy as np
import pytest

from pyoracle import TYPE_FLOAT, params_precision
from test_gpu_region import (LIB_HIP, SENTINEL, TYPES, _arr4, _blocks, _export, _guarded, _int_field, _job, _params,
                             _special_field)

pytestmark = pytest.mark.gpu

SHAPE = (20, 24, 37)  # 5 x 6 x 10 blocks, a partial edge in x
WHOLE = ((0, 20), (0, 24), (0, 37))
BATCH = [
    ((0, 1), (0, 1), (0, 1)),        # 1 block
    ((0, 16), (0, 16), (0, 16)),     # 64 blocks: one full wave
    ((0, 20), (0, 13), (0, 4)),      # 5 * 4 * 1 = 20 blocks
    ((0, 16), (0, 20), (0, 16)),     # 4 * 5 * 4 = 80 blocks: two waves
    WHOLE,                           # 300 blocks: five waves, two workgroups
    ((3, 18), (5, 22), (2, 35)),     # unaligned on every side
]
MODES = [("rate", 16), ("rate", 3.25), ("precision", 20), ("reversible", None)]


class Region(ctypes.Structure):
    """zfp_hip_region (include/zfp_hip.h)."""
    _fields_ = [("lo", ctypes.c_uint64 * 4), ("hi", ctypes.c_uint64 * 4), ("dst", ctypes.c_void_p),
                ("dst_stride", ctypes.c_int64 * 4)]


@pytest.fixture(scope="module")
def hip(product):
    lib = ctypes.CDLL(LIB_HIP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.zfp_hip_decompress_regions.restype = ctypes.c_int
    lib.zfp_hip_decompress_regions.argtypes = [vp, vp, u64, vp, u64, u64, ctypes.c_int, vp, vp]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture(scope="module")
def coded(oracle):
    """{(mode, param): (words, ref, params)} of the default float32 field, coded and decoded by the oracle once."""
    out = {}
    for mode, param in MODES:
        rng = np.random.default_rng(zlib.crc32(repr((mode, param)).encode()))
        a = _special_field(SHAPE, np.float32, rng)
        params = _params(mode, param, TYPE_FLOAT, 3)
        words, _ = oracle.compress_words(a, params)
        ref, _ = oracle.decompress_words(words, SHAPE, np.float32, params)
        ref.setflags(write=False)
        out[(mode, param)] = (words, ref, params)
    return out


def _table(regions, ptrs, strides):
    """The zfp_hip_region array; regions, strides in numpy axis order."""
    arr = (Region * len(regions))()
    for r, region, ptr, st in zip(arr, regions, ptrs, strides):
        r.lo = _arr4(ctypes.c_uint64, [lo for lo, _ in region])
        r.hi = _arr4(ctypes.c_uint64, [hi for _, hi in region])
        r.dst = ptr
        r.dst_stride = _arr4(ctypes.c_int64, st)
    return arr


def _call(hip, job, regions, ptrs, strides, words_ptr, nwords, bit_offset=0, index=None):
    blocks = ctypes.c_uint64(12345)
    rc = hip.zfp_hip_decompress_regions(ctypes.byref(job), _table(regions, ptrs, strides), len(regions), words_ptr,
                                        nwords, bit_offset, -1, index, ctypes.byref(blocks))
    return rc, blocks.value


def _check(hip, words, shape, dtype, params, ref, regions, *, coded_box=None, bit_offset=0, index=None, ztype=None,
           layouts=None, dev_dst=False, dev_stream=False):
    """One batch into guarded views: (i) bytes, (ii) guards, (iii) blocks_read."""
    dtype = np.dtype(dtype)
    job = _job(shape, ztype or TYPES[dtype], params, coded_box)
    layouts = layouts or [_guarded] * len(regions)
    dests = [lay([hi - lo for lo, hi in region], dtype) for lay, region in zip(layouts, regions)]
    strides = [[s // dtype.itemsize for s in view.strides] for _, view in dests]
    keep = []
    if dev_dst or dev_stream:
        import torch
    if dev_dst:
        keep = [torch.from_numpy(big).cuda() for big, _ in dests]
        ptrs = [d.data_ptr() + (view.ctypes.data - big.ctypes.data) for d, (big, view) in zip(keep, dests)]
    else:
        ptrs = [view.ctypes.data for _, view in dests]
    wptr = words.ctypes.data
    if dev_stream:
        d_words = torch.from_numpy(words.view(np.int64).copy()).cuda()
        wptr = d_words.data_ptr()
    rc, got = _call(hip, job, regions, ptrs, strides, wptr, len(words), bit_offset, index)
    assert rc == 1, hip.zfp_hip_last_error().decode()
    if dev_dst:
        torch.cuda.synchronize()
        for d, (big, _) in zip(keep, dests):
            big[...] = d.cpu().numpy()
    for i, (region, (big, view)) in enumerate(zip(regions, dests)):
        want = ref[tuple(slice(lo, hi) for lo, hi in region)]
        assert np.ascontiguousarray(view).tobytes() == np.ascontiguousarray(want).tobytes(), (i, region, "values")
        view[...] = np.frombuffer(bytes([SENTINEL]) * dtype.itemsize, dtype=dtype)[0]  # (any strides)
        assert (big.view(np.uint8) == SENTINEL).all(), (i, region, "guard band written")
    assert got == sum(_blocks(region, coded_box, shape) for region in regions), "blocks_read"


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,param", MODES)
def test_one_region_the_whole_field(hip, coded, mode, param):
    words, ref, params = coded[(mode, param)]
    _check(hip, words, SHAPE, np.float32, params, ref, [WHOLE])


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("mode,param", MODES)
def test_batch_of_mixed_sizes(hip, coded, mode, param, order):
    words, ref, params = coded[(mode, param)]
    _check(hip, words, SHAPE, np.float32, params, ref, BATCH if order == "forward" else BATCH[::-1])


@pytest.mark.parametrize("mode,param", MODES)
def test_seventy_single_elements(hip, coded, mode, param):
    """More regions than a wave has lanes: 70 waves in 18 workgroups."""
    words, ref, params = coded[(mode, param)]
    rng = np.random.default_rng(70)
    regions = [tuple((int(c), int(c) + 1) for c in (rng.integers(0, n) for n in SHAPE)) for _ in range(70)]
    _check(hip, words, SHAPE, np.float32, params, ref, regions)


@pytest.mark.parametrize("mode,param", [("rate", 16), ("precision", 20)])
def test_repeated_and_overlapping_regions(hip, coded, mode, param):
    words, ref, params = coded[(mode, param)]
    r = ((3, 18), (5, 22), (2, 35))
    _check(hip, words, SHAPE, np.float32, params, ref, [r, r])
    _check(hip, words, SHAPE, np.float32, params, ref, [((0, 12), (2, 14), (0, 21)), ((7, 20), (9, 24), (13, 37))])


# ---- per-region layouts in one batch ----
def _dense_aligned(ext, dtype):
    """Dense, 16 bytes into a 16-byte aligned buffer (row stores when lo[0] is a block boundary)."""
    n = int(np.prod(ext))
    pad = 16 // np.dtype(dtype).itemsize
    raw = np.empty((n + 2 * pad) * np.dtype(dtype).itemsize + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    big = raw[off: off + (n + 2 * pad) * np.dtype(dtype).itemsize].view(dtype)
    big.view(np.uint8)[...] = SENTINEL
    view = big[pad: pad + n].reshape(ext)
    assert view.ctypes.data % 16 == 0
    return big, view


def _offset_by_one(ext, dtype):
    """Dense, one element past a 16-byte boundary (scalar stores)."""
    big, view = _dense_aligned(ext, dtype)
    pad = 16 // np.dtype(dtype).itemsize
    return big, big[pad + 1: pad + 1 + view.size].reshape(ext)


def _x_stride_2(ext, dtype):
    full = list(ext)
    full[-1] = 2 * ext[-1] + 8
    big = np.empty([n + 2 for n in full[:-1]] + [full[-1]], dtype=dtype)
    big.view(np.uint8)[...] = SENTINEL
    idx = tuple(slice(1, 1 + n) for n in ext[:-1]) + (slice(3, 3 + 2 * ext[-1], 2),)
    return big, big[idx]


def _negative_y(ext, dtype):
    big, view = _guarded(ext, dtype)
    return big, view[..., ::-1, :]


@pytest.mark.parametrize("mode,param", [("rate", 16), ("reversible", None)])
def test_layouts_differ_per_region(hip, coded, mode, param):
    words, ref, params = coded[(mode, param)]
    regions = [((4, 20), (8, 24), (4, 20)),   # dense, aligned, lo[0] a block boundary: row stores
               ((3, 18), (5, 22), (2, 35)),   # x stride 2
               ((0, 16), (0, 20), (0, 16)),   # negative y stride
               ((4, 20), (8, 24), (4, 20))]   # dense, one element past a 16-byte boundary
    _check(hip, words, SHAPE, np.float32, params, ref, regions,
           layouts=[_dense_aligned, _x_stride_2, _negative_y, _offset_by_one])


# ---- host and device memory ----
@pytest.mark.parametrize("dev_stream,dev_dst", [(True, True), (False, False), (True, False)],
                         ids=["device-device", "host-host", "device stream-host dst"])
@pytest.mark.parametrize("mode,param", [("rate", 16), ("precision", 20)])
def test_host_and_device_memory(hip, coded, mode, param, dev_stream, dev_dst):
    words, ref, params = coded[(mode, param)]
    _check(hip, words, SHAPE, np.float32, params, ref, BATCH, dev_dst=dev_dst, dev_stream=dev_stream)


def test_mixed_destinations_are_refused(hip, coded):
    import torch
    words, _, params = coded[("rate", 16)]
    job = _job(SHAPE, TYPE_FLOAT, params)
    regions = [((0, 4), (0, 4), (0, 4))] * 3
    host = [np.full(64, SENTINEL, dtype=np.uint8).view(np.float32) for _ in range(2)]
    dev = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")
    ptrs = [host[0].ctypes.data, dev.data_ptr(), host[1].ctypes.data]
    rc, blocks = _call(hip, job, regions, ptrs, [[16, 4, 1]] * 3, words.ctypes.data, len(words))
    assert rc == 0 and blocks == 12345
    assert "regions[1]" in hip.zfp_hip_last_error().decode()
    torch.cuda.synchronize()
    assert all((h.view(np.uint8) == SENTINEL).all() for h in host) and bool((dev == 7.0).all())


# ---- a chunk's stream behind a header ----
@pytest.mark.parametrize("mode,param", [("rate", 8), ("precision", 20)])
def test_coded_chunk_at_a_bit_offset(hip, oracle, mode, param):
    shape = (24, 24, 48)
    box_np = [(8, 20), (4, 24), (12, 40)]
    rng = np.random.default_rng(3)
    a = _special_field(shape, np.float32, rng)
    params = _params(mode, param, TYPE_FLOAT, 3)
    box = list(reversed(box_np)) + [(0, 0)]
    words, _ = oracle.compress_words(a, params, box=box, bit_offset=96)
    ref, _ = oracle.decompress_words(words, shape, np.float32, params, box=box, bit_offset=96)
    regions = [((8, 13), (4, 11), (12, 30)), ((10, 19), (9, 22), (17, 39)), tuple(box_np), ((19, 20), (23, 24), (39, 40))]
    _check(hip, words, shape, np.float32, params, ref, regions, coded_box=box_np, bit_offset=96)


# ---- variable rate: the index ----
def test_index_handling(hip, product, oracle):
    """The encoder's index (no scan), no index (scanned, not stale), and an index
    of another stream of the same shape that passes the fingerprint: the block
    lengths catch it and the whole batch is decoded again with a scan."""
    lib = product.lib
    rng = np.random.default_rng(17)
    a = _special_field(SHAPE, np.float32, rng)
    b = _special_field(SHAPE, np.float32, rng)
    params = params_precision(20)
    wa, _ = oracle.compress_words(a, params)
    wb, _ = oracle.compress_words(b, params)
    ra, _ = oracle.decompress_words(wa, SHAPE, np.float32, params)
    assert product.compress(a, "precision", 20) == wa.tobytes()
    ia = product.last_index
    assert product.compress(b, "precision", 20) == wb.tobytes()
    ib = product.last_index
    product.last_index = None
    try:
        _check(hip, wa, SHAPE, np.float32, params, ra, BATCH, index=ia)
        assert product.last_scan() is None and lib.zfp_hip_last_stale_index() == 0
        _check(hip, wa, SHAPE, np.float32, params, ra, BATCH)
        assert product.last_scan() is not None and lib.zfp_hip_last_stale_index() == 0
        ea, eb = _export(lib, ia), _export(lib, ib)
        eb[24:32] = ea[24:32]  # total bits
        eb[48:56] = ea[48:56]  # fingerprint
        wrong = lib.zfp_hip_index_import(bytes(eb), len(eb))
        assert wrong
        _check(hip, wa, SHAPE, np.float32, params, ra, BATCH, index=wrong)
        assert lib.zfp_hip_last_stale_index() == 1 and product.last_scan() is not None
        lib.zfp_hip_index_free(wrong)
    finally:
        lib.zfp_hip_index_free(ia)
        lib.zfp_hip_index_free(ib)


# ---- other dimensionalities and types ----
@pytest.mark.parametrize("dtype,shape,regions", [
    (np.float32, (37,), [((0, 37),), ((3, 30),), ((36, 37),)]),
    (np.float32, (24, 37), [((0, 24), (0, 37)), ((2, 23), (5, 34)), ((8, 12), (0, 37)), ((23, 24), (36, 37))]),
    (np.float64, SHAPE, BATCH),
], ids=["1d-f32", "2d-f32", "3d-f64"])
@pytest.mark.parametrize("mode,param", [("rate", 8), ("reversible", None)])
def test_other_dimensionalities_and_double(hip, oracle, dtype, shape, regions, mode, param):
    rng = np.random.default_rng(29)
    a = (rng.standard_normal(shape) * 100).astype(dtype)
    params = _params(mode, param, TYPES[np.dtype(dtype)], len(shape))
    words, _ = oracle.compress_words(a, params)
    ref, _ = oracle.decompress_words(words, shape, dtype, params)
    _check(hip, words, shape, dtype, params, ref, regions)


@pytest.mark.parametrize("mode,param", [("rate", 8), ("reversible", None)])
def test_int32_3d_matches_reference(hip, ref_capi, mode, param):
    """The oracle codes floats only: the stream and the expected values are the
    reference library's, as in test_gpu_types.py."""
    a = _int_field(SHAPE, np.int32, 31)
    data = ref_capi.compress(a, mode, param, ztype=1)
    ref, _ = ref_capi.decompress(data, SHAPE, np.int32, mode, param, ztype=1)
    words = np.frombuffer(data + bytes((-len(data)) % 8), dtype=np.uint64).copy()
    _check(hip, words, SHAPE, np.int32, _params(mode, param, 1, 3), ref, BATCH)


# ---- zfpy ----
@pytest.mark.parametrize("mode,kw", [(("rate", 8), dict(rate=8)), (("precision", 20), dict(precision=20))])
def test_zfpy_decompress_regions(oracle, mode, kw):
    import zfpy
    rng = np.random.default_rng(41)
    a = rng.standard_normal(SHAPE).astype(np.float32)
    params = _params(mode[0], mode[1], TYPE_FLOAT, 3)
    words, _ = oracle.compress_words(a, params)
    ref, _ = oracle.decompress_words(words, SHAPE, np.float32, params)
    s = zfpy.compress_numpy(a, **kw)
    # list form
    regions = [(slice(3, 18), slice(5, 22), slice(2, 35)), (None, slice(None), slice(36, 37)), None]
    got = zfpy.decompress_regions(s, regions)
    assert len(got) == 3
    for g, r in zip(got, regions):
        sl = tuple(slice(None) if x is None else x for x in (r if r is not None else (None,) * 3))
        want = np.ascontiguousarray(ref[sl])
        assert g.flags.c_contiguous and g.shape == want.shape and g.tobytes() == want.tobytes(), r
    # stacked crops: the rows of a (N, d, h, w) array
    corners = [(0, 0, 0), (12, 16, 29), (5, 9, 13), (8, 8, 8)]
    crops = [tuple(slice(c, c + 8) for c in corner) for corner in corners]
    batch = np.full((4, 8, 8, 8), 7.0, dtype=np.float32)
    ret = zfpy.decompress_regions(s, crops, out=list(batch))
    assert len(ret) == 4 and all(np.shares_memory(r, batch) for r in ret)
    for k, crop in enumerate(crops):
        assert batch[k].tobytes() == np.ascontiguousarray(ref[crop]).tobytes(), crop
    with pytest.raises(ValueError):
        zfpy.decompress_regions(s, crops, out=list(batch[:3]))
    with pytest.raises(TypeError):
        zfpy.decompress_regions(s, crops, out=list(batch.astype(np.float64)))


@pytest.mark.parametrize("mode,kw", [(("rate", 8), dict(rate=8)), (("precision", 16), dict(precision=16))])
def test_zfp_parallel_decompress_regions(oracle, mode, kw):
    import zfpy
    shape = (16, 32, 48)
    rng = np.random.default_rng(43)
    idx = np.indices(shape, dtype=np.float32)
    a = (np.sin(0.05 * idx[0]) + np.cos(0.07 * idx[1]) * np.sin(0.03 * idx[2])
         + 1e-3 * rng.standard_normal(shape)).astype(np.float32)
    zp = zfpy.zfp_parallel(shape, "float32", nparts=8)
    zp.get_numpy_array()[...] = a
    zp.compress(nthreads=8, **kw)
    boxes = zp.get_chunkit().boxes
    assert len(boxes) == 8
    # expected: every chunk coded and decoded by the oracle
    params = _params(mode[0], mode[1], TYPE_FLOAT, 3)
    full = np.empty(shape, dtype=np.float32)
    for b in boxes:
        box = [tuple(b[k]) for k in range(3)] + [(0, 0)]
        words, _ = oracle.compress_words(a, params, box=box)
        ref, _ = oracle.decompress_words(words, shape, np.float32, params, box=box)
        sl = tuple(slice(b[k][0], b[k][1]) for k in (2, 1, 0))
        full[sl] = ref[sl]
    zp.get_numpy_array()[...] = 7.0
    x, y, z = boxes[3][:3]  # one chunk's box (x first)
    regions = [(slice(1, 15), slice(3, 30), slice(5, 45)),                                        # crosses every cut
               (slice(z[0] + 1, z[1] - 1), slice(y[0] + 2, y[1] - 1), slice(x[0] + 3, x[1] - 2)),  # in one chunk
               (slice(7, 8), None, slice(0, 48))]
    lo, hi = (5, 3, 1), (45, 30, 15)
    assert all(all(lo[k] < b[k][1] and b[k][0] < hi[k] for k in range(3)) for b in boxes)
    got = zp.decompress_regions(regions, nthreads=8)
    assert (zp.get_numpy_array() == 7.0).all(), "decompress_regions touched the shared array"
    assert len(got) == 3
    for g, r in zip(got, regions):
        r = tuple(slice(None) if s is None else s for s in r)
        assert g.tobytes() == np.ascontiguousarray(full[r]).tobytes(), r
