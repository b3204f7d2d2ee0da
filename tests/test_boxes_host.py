"""Batched region decode without a GPU: exports, validation, the kernels' descriptors.

Every validation failure of zfp_hip_decompress_regions / zfp_decompress_regions
is decided before any GPU call, returns 0 and leaves every destination and
*blocks_read untouched, so these run on a machine without a GPU.  The batched
kernel has the 26 instantiations of decode3_region, which keeps its own, and its
float 3D lossy instantiation keeps its plane registers in VGPRs (private
segment 0); the descriptors are read from libzfp_hip.so as test_region_host.py
reads them.
"""
import ctypes
import re

import numpy as np
import pytest

from kdesc import _kernel_scratch
from test_region_host import LIB_HIP, LIB_ZFP, SENTINEL, _exports, _job


class Region(ctypes.Structure):
    """zfp_hip_region (include/zfp_hip.h)."""
    _fields_ = [("lo", ctypes.c_uint64 * 4), ("hi", ctypes.c_uint64 * 4), ("dst", ctypes.c_void_p),
                ("dst_stride", ctypes.c_int64 * 4)]


def test_libraries_export_the_batched_entry_points():
    assert "zfp_decompress_regions" in _exports(LIB_ZFP)
    assert "zfp_hip_decompress_regions" in _exports(LIB_HIP)


@pytest.fixture(scope="module")
def hip():
    lib = ctypes.CDLL(LIB_HIP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.zfp_hip_decompress_regions.restype = ctypes.c_int
    lib.zfp_hip_decompress_regions.argtypes = [vp, vp, u64, vp, u64, u64, ctypes.c_int, vp, vp]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


def _regions(boxes, outs):
    """boxes: [(lo, hi)] with x first; outs: one uint8 array per box (None: a null destination)."""
    arr = (Region * max(len(boxes), 1))()
    for r, (lo, hi), out in zip(arr, boxes, outs):
        for a in range(len(lo)):
            r.lo[a], r.hi[a] = lo[a], hi[a]
        r.dst = out.ctypes.data if out is not None else None
        r.dst_stride[0], r.dst_stride[1], r.dst_stride[2], r.dst_stride[3] = 1, 4, 16, 64
    return arr


GOOD = ((0, 0, 0), (4, 4, 4))
BOX = dict(f=(4, 0, 8), e=(16, 12, 20))
# (name, job, boxes, nulls, nregions or None for len(boxes), text the message must hold)
CASES = [
    ("null job", None, [GOOD], (), None, None),
    ("null regions", _job(3, (16, 16, 16)), [GOOD], ("regions",), None, None),
    ("null words", _job(3, (16, 16, 16)), [GOOD], ("words",), None, None),
    ("null dst in an entry", _job(3, (16, 16, 16)), [GOOD, GOOD, GOOD], ("dst1",), None, "regions[1]"),
    ("empty region", _job(3, (16, 16, 16)), [GOOD, ((0, 5, 0), (4, 5, 4)), GOOD], (), None, "entry 2 of 3"),
    ("reversed region", _job(3, (16, 16, 16)), [GOOD, GOOD, ((0, 0, 9), (4, 4, 3))], (), None, "entry 3 of 3"),
    ("below the coded box", _job(3, (24, 24, 24), **BOX), [((4, 0, 8), (8, 4, 12)), ((3, 0, 8), (8, 4, 12)),
                                                           ((4, 0, 8), (8, 4, 12))], (), None, "entry 2 of 3"),
    ("past the coded box", _job(3, (24, 24, 24), **BOX), [((4, 0, 8), (8, 4, 21))], (), None, "entry 1 of 1"),
    ("past the field", _job(1, (10,)), [((0,), (4,)), ((2,), (11,)), ((0,), (4,))], (), None, "entry 2 of 3"),
    ("4D", _job(4, (8, 8, 8, 8)), [((0, 0, 0, 0), (4, 4, 4, 4))], (), None, "4D"),
    ("too many regions", _job(3, (16, 16, 16)), [GOOD], (), 65537, "65537"),
]


@pytest.mark.parametrize("name,job,boxes,nulls,nregions,text", CASES, ids=[c[0] for c in CASES])
def test_validation_failures_return_0_and_leave_the_destinations(hip, name, job, boxes, nulls, nregions, text):
    outs = [np.full(4096, SENTINEL, dtype=np.uint8) for _ in boxes]
    words = np.zeros(4096, dtype=np.uint64)
    blocks = ctypes.c_uint64(12345)
    given = [None if "dst%d" % i in nulls else o for i, o in enumerate(outs)]
    if nregions is not None:  # the count alone decides: every entry of the table itself is a good one
        arr = (Region * nregions)()
        for r in arr:
            r.lo[0] = r.lo[1] = r.lo[2] = 0
            r.hi[0] = r.hi[1] = r.hi[2] = 4
            r.dst = outs[0].ctypes.data
            r.dst_stride[0], r.dst_stride[1], r.dst_stride[2] = 1, 4, 16
    else:
        arr = _regions(boxes, given)
    rc = hip.zfp_hip_decompress_regions(
        ctypes.byref(job) if job is not None else None, None if "regions" in nulls else arr,
        nregions if nregions is not None else len(boxes), None if "words" in nulls else words.ctypes.data,
        len(words), 0, -1, None, ctypes.byref(blocks))
    assert rc == 0, name
    msg = hip.zfp_hip_last_error().decode()
    assert msg and "no HIP device" not in msg, (name, msg)
    if text:
        assert text in msg, (name, msg)
    assert all((o == SENTINEL).all() for o in outs), name
    assert blocks.value == 12345, name


def test_the_padded_total_is_bounded(hip):
    """Sum of 64 ceil(nrblocks / 64) above 2^32 - 1: 65 regions, each the whole
    of a box of 2^26 blocks (2^26 lanes each, 65 * 2^26 > 2^32), fail before any
    GPU call; the message speaks of lanes."""
    n = (1 << 11, 1 << 11, 1 << 10)  # 2^9 * 2^9 * 2^8 blocks
    out = np.full(64, SENTINEL, dtype=np.uint8)
    words = np.zeros(8, dtype=np.uint64)
    blocks = ctypes.c_uint64(12345)
    arr = _regions([((0, 0, 0), n)] * 65, [out] * 65)
    rc = hip.zfp_hip_decompress_regions(ctypes.byref(_job(3, n)), arr, 65, words.ctypes.data, len(words), 0, -1, None,
                                        ctypes.byref(blocks))
    assert rc == 0
    msg = hip.zfp_hip_last_error().decode()
    assert "lanes" in msg and "no HIP device" not in msg, msg
    assert (out == SENTINEL).all() and blocks.value == 12345


def test_no_regions_is_a_success_without_a_gpu_call(hip):
    words = np.zeros(64, dtype=np.uint64)
    blocks = ctypes.c_uint64(12345)
    arr = (Region * 1)()
    rc = hip.zfp_hip_decompress_regions(ctypes.byref(_job(3, (16, 16, 16))), arr, 0, words.ctypes.data, len(words), 0,
                                        -1, None, ctypes.byref(blocks))
    assert rc == 1, hip.zfp_hip_last_error().decode()
    assert blocks.value == 0


def test_host_api_refuses_a_mismatch_in_the_second_pair(prod):
    """zfp_decompress_regions: the second `out` of another scalar type, or of
    extents that are not its region's, returns 0 and writes nothing -- to the
    first, matching, destination either."""
    lib = prod.lib
    lib.zfp_decompress_regions.restype = ctypes.c_int
    lib.zfp_decompress_regions.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]

    class Chunk(ctypes.Structure):
        _fields_ = [(k, ctypes.c_size_t) for k in ("fx", "fy", "fz", "fw", "ex", "ey", "ez", "ew")]

    words = np.zeros(4096, dtype=np.uint64)
    bs = lib.stream_open(words.ctypes.data, words.nbytes)
    zs = lib.zfp_stream_open(bs)
    lib.zfp_stream_set_rate(zs, 8.0, 3, 3, 0)
    lib.zfp_stream_rewind(zs)
    field = lib.zfp_field_3d(None, 3, 16, 12, 8)
    regions = (Chunk * 2)(Chunk(fx=0, fy=0, fz=0, ex=4, ey=4, ez=4),
                          Chunk(fx=2, fy=3, fz=1, ex=10, ey=9, ez=5))  # extents (4, 4, 4) and (8, 6, 4)
    try:
        for ztype, ext in ((4, (8, 6, 4)), (3, (8, 6, 5)), (3, (7, 6, 4))):
            first = np.full(4 * 4 * 4 * 4, SENTINEL, dtype=np.uint8)
            second = np.full(8 * 6 * 5 * 8, SENTINEL, dtype=np.uint8)
            ofields = (ctypes.c_void_p * 2)(lib.zfp_field_3d(first.ctypes.data, 3, 4, 4, 4),
                                            lib.zfp_field_3d(second.ctypes.data, ztype, *ext))
            assert lib.zfp_decompress_regions(zs, field, None, regions, 2, ofields) == 0, (ztype, ext)
            for f in ofields:
                lib.zfp_field_free(f)
            assert (first == SENTINEL).all() and (second == SENTINEL).all(), (ztype, ext)
        assert lib.stream_rtell(bs) == 0
    finally:
        lib.zfp_field_free(field)
        lib.zfp_stream_close(zs)
        lib.stream_close(bs)


def test_batched_kernels_and_their_scratch():
    sc = _kernel_scratch(open(LIB_HIP, "rb").read())
    boxes = {k: v for k, v in sc.items() if k.startswith("_ZN7zfp_amd13decode3_boxesI")}
    assert len(boxes) == 26, sorted(boxes)  # every type, dimensionality and mode the host can select
    hot = {k: v for k, v in boxes.items() if re.match(r"_ZN7zfp_amd13decode3_boxesIfLb0ELb0ELi3EE", k)}
    assert len(hot) == 1 and all(v == 0 for v in hot.values()), hot
    region = [k for k in sc if k.startswith("_ZN7zfp_amd14decode3_regionI")]
    assert len(region) == 26, sorted(region)
