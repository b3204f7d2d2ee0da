"""Batched region encode without a GPU: exports, validation, the kernels' descriptors.

Every validation failure of zfp_hip_compress_regions / zfp_compress_regions is
decided before any GPU call, returns 0 and leaves the stream and
*blocks_written untouched, so these run on a machine without a GPU.  The
batched kernel has the 13 instantiations of encode3_region, which keeps its
own; its float 3D instantiation uses no scratch and the VGPRs recorded in
DESIGN 3.14 (the descriptors are read from libzfp_hip.so by kdesc.py and
test_encode_full16_resources.py's reader).
"""
import ctypes
import struct

import numpy as np
import pytest

from kdesc import _kernel_scratch
from test_encode_full16_resources import _descriptor
from test_region_encode_host import LIB_HIP, LIB_ZFP, SENTINEL, _variable
from test_region_host import BOX, _exports, _job


class SrcRegion(ctypes.Structure):
    """zfp_hip_src_region (include/zfp_hip.h)."""
    _fields_ = [("lo", ctypes.c_uint64 * 4), ("hi", ctypes.c_uint64 * 4), ("src", ctypes.c_void_p),
                ("src_stride", ctypes.c_int64 * 4)]


def test_libraries_export_the_batched_encode_entry_points():
    assert "zfp_compress_regions" in _exports(LIB_ZFP)
    assert "zfp_hip_compress_regions" in _exports(LIB_HIP)


@pytest.fixture(scope="module")
def hip():
    lib = ctypes.CDLL(LIB_HIP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.zfp_hip_compress_regions.restype = ctypes.c_int
    lib.zfp_hip_compress_regions.argtypes = [vp, vp, u64, vp, u64, u64, ctypes.c_int, vp]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


def _regions(boxes, srcs):
    """boxes: [(lo, hi)] with x first; srcs: one array per box (None: a null source)."""
    arr = (SrcRegion * max(len(boxes), 1))()
    for r, (lo, hi), src in zip(arr, boxes, srcs):
        for a in range(len(lo)):
            r.lo[a], r.hi[a] = lo[a], hi[a]
        r.src = src.ctypes.data if src is not None else None
        r.src_stride[0], r.src_stride[1], r.src_stride[2], r.src_stride[3] = 1, 16, 256, 4096
    return arr


GOOD = ((0, 0, 0), (4, 4, 4))
G2 = ((4, 0, 0), (8, 4, 4))
G3 = ((8, 8, 8), (16, 16, 16))
J16 = (3, (16, 16, 16))
# (name, job, boxes, nulls, nregions or None for len(boxes), capacity words or None, texts the message must hold)
CASES = [
    ("null job", None, [GOOD], (), None, None, ()),
    ("null regions", _job(*J16), [GOOD], ("regions",), None, None, ()),
    ("null words", _job(*J16), [GOOD], ("words",), None, None, ()),
    ("null src in an entry", _job(*J16), [GOOD, G2, G3], ("src1",), None, None, ("regions[1]",)),
    ("empty region", _job(*J16), [GOOD, ((0, 5, 0), (4, 5, 4)), G3], (), None, None, ("entry 2 of 3",)),
    ("reversed region", _job(*J16), [GOOD, G2, ((0, 0, 9), (4, 4, 3))], (), None, None, ("entry 3 of 3",)),
    ("below the coded box", _job(3, (24, 24, 24), **BOX), [((4, 0, 8), (8, 4, 12)), ((3, 4, 8), (8, 8, 12)),
                                                           ((8, 0, 8), (12, 4, 12))], (), None, None,
     ("entry 2 of 3",)),
    ("past the coded box", _job(3, (24, 24, 24), **BOX), [((4, 0, 8), (8, 4, 21))], (), None, None,
     ("entry 1 of 1",)),
    ("past the field", _job(1, (10,)), [((0,), (4,)), ((2,), (11,)), ((4,), (8,))], (), None, None,
     ("entry 2 of 3",)),
    ("4D", _job(4, (8, 8, 8, 8)), [((0, 0, 0, 0), (4, 4, 4, 4))], (), None, None, ("4D",)),
    ("variable rate: precision", _variable(_job(*J16)), [GOOD, G2], (), None, None, ("fixed-rate",)),
    ("variable rate: accuracy", _variable(_job(*J16), maxprec=64, minexp=-10), [GOOD], (), None, None,
     ("fixed-rate",)),
    ("variable rate: reversible", _variable(_job(*J16), maxprec=64, minexp=-1075), [GOOD], (), None, None,
     ("fixed-rate",)),
    ("variable rate: minbits < maxbits", _variable(_job(*J16), 256, 512, 64), [GOOD], (), None, None,
     ("fixed-rate",)),
    ("too many regions", _job(*J16), [GOOD], (), 65537, None, ("65537",)),
    # 16^3 at rate 8: 64 blocks of 8 words; the last block of G3 is block 63, needed by the middle entry
    ("stream ends before the highest needed block", _job(*J16), [GOOD, G3, G2], (), None, 511, ("regions[1]",)),
    ("stream ends inside the first block", _job(*J16), [GOOD], (), None, 7, ()),
    ("empty stream", _job(*J16), [GOOD, G2], (), None, 0, ()),
    ("capacity that wraps around", _job(*J16), [GOOD], (), None, (1 << 64) - 1, ()),
    # the elements are disjoint, the block [0:4, 0:4, 0:4] is not
    ("two entries in one block", _job(*J16), [G3, ((0, 0, 0), (2, 4, 4)), G2, ((2, 0, 0), (4, 4, 4))], (), None, None,
     ("regions[1]", "regions[3]", "disjoint")),
    ("identical entries", _job(*J16), [GOOD, G2, GOOD], (), None, None, ("regions[0]", "regions[2]")),
    ("nested entries", _job(*J16), [((0, 0, 0), (16, 16, 16)), ((5, 6, 7), (6, 7, 8))], (), None, None,
     ("regions[0]", "regions[1]")),
    ("blocks count from the coded box's origin", _job(3, (24, 24, 24), **BOX),
     [((4, 0, 8), (7, 4, 12)), ((7, 0, 8), (12, 4, 12))], (), None, None, ("regions[0]", "regions[1]")),
    ("1D neighbours inside one block", _job(1, (64,)), [((0,), (6,)), ((6,), (20,))], (), None, None,
     ("regions[0]", "regions[1]")),
    ("2D corner block", _job(2, (16, 16)), [((0, 0), (8, 8)), ((7, 7), (16, 16))], (), None, None,
     ("regions[0]", "regions[1]")),
]


@pytest.mark.parametrize("name,job,boxes,nulls,nregions,cap,texts", CASES, ids=[c[0] for c in CASES])
def test_validation_failures_return_0_and_leave_the_stream(hip, name, job, boxes, nulls, nregions, cap, texts):
    srcs = [np.zeros(4096, dtype=np.float32) for _ in boxes]
    words = np.full(4096, SENTINEL, dtype=np.uint8).view(np.uint64)
    blocks = ctypes.c_uint64(12345)
    given = [None if "src%d" % i in nulls else s for i, s in enumerate(srcs)]
    if nregions is not None:  # the count alone decides: the table's entries are good and pairwise disjoint in x
        arr = (SrcRegion * nregions)()
        for r in arr:
            r.lo[0] = r.lo[1] = r.lo[2] = 0
            r.hi[0] = r.hi[1] = r.hi[2] = 4
            r.src = srcs[0].ctypes.data
            r.src_stride[0], r.src_stride[1], r.src_stride[2] = 1, 4, 16
    else:
        arr = _regions(boxes, given)
    rc = hip.zfp_hip_compress_regions(
        ctypes.byref(job) if job is not None else None, None if "regions" in nulls else arr,
        nregions if nregions is not None else len(boxes), None if "words" in nulls else words.ctypes.data,
        len(words) if cap is None else cap, 0 if cap != (1 << 64) - 1 else (1 << 64) - 64, -1, ctypes.byref(blocks))
    assert rc == 0, name
    msg = hip.zfp_hip_last_error().decode()
    assert msg and "no HIP device" not in msg, (name, msg)
    for t in texts:
        assert t in msg, (name, msg)
    assert (words.view(np.uint8) == SENTINEL).all(), name
    assert blocks.value == 12345, name


def test_face_neighbours_are_not_an_overlap(hip):
    """Block-aligned neighbours share no block: the refusal, if any, is not the
    disjointness rule's (without a GPU the call stops at the device count)."""
    srcs = [np.zeros(4096, dtype=np.float32) for _ in range(3)]
    words = np.full(4096, SENTINEL, dtype=np.uint8).view(np.uint64)
    arr = _regions([GOOD, G2, ((0, 4, 0), (8, 8, 4))], srcs)
    rc = hip.zfp_hip_compress_regions(ctypes.byref(_job(*J16)), arr, 3, words.ctypes.data, len(words), 0, -1, None)
    if rc == 0:
        assert "no HIP device" in hip.zfp_hip_last_error().decode()


def test_a_bit_offset_counts_towards_the_capacity(hip):
    """64 blocks of 512 bits behind 96 header bits need 514 words, not 513."""
    srcs = [np.zeros(4096, dtype=np.float32) for _ in range(2)]
    words = np.full(514 * 8, SENTINEL, dtype=np.uint8).view(np.uint64)
    arr = _regions([G3, GOOD], srcs)
    rc = hip.zfp_hip_compress_regions(ctypes.byref(_job(*J16)), arr, 2, words.ctypes.data, 513, 96, -1, None)
    assert rc == 0
    msg = hip.zfp_hip_last_error().decode()
    assert "end before bit" in msg and "no HIP device" not in msg, msg
    assert (words.view(np.uint8) == SENTINEL).all()


def test_the_padded_total_is_bounded(hip):
    """Sum of 64 ceil(nrblocks / 64) above 2^32 - 1: 65 entries, each the whole
    of a box of 2^26 blocks, fail on the lane count (which is checked entry by
    entry, before the batch's disjointness)."""
    n = (1 << 11, 1 << 11, 1 << 10)
    src = np.zeros(64, dtype=np.float32)
    words = np.full(8, SENTINEL, dtype=np.uint8).view(np.uint64)
    blocks = ctypes.c_uint64(12345)
    arr = _regions([((0, 0, 0), n)] * 65, [src] * 65)
    rc = hip.zfp_hip_compress_regions(ctypes.byref(_job(3, n)), arr, 65, words.ctypes.data, len(words), 0, -1,
                                      ctypes.byref(blocks))
    assert rc == 0
    msg = hip.zfp_hip_last_error().decode()
    assert "lanes" in msg and "no HIP device" not in msg, msg
    assert (words.view(np.uint8) == SENTINEL).all() and blocks.value == 12345


def test_no_regions_is_a_success_without_a_gpu_call(hip):
    words = np.full(64, SENTINEL, dtype=np.uint8).view(np.uint64)
    blocks = ctypes.c_uint64(12345)
    arr = (SrcRegion * 1)()
    rc = hip.zfp_hip_compress_regions(ctypes.byref(_job(*J16)), arr, 0, words.ctypes.data, len(words), 0, -1,
                                      ctypes.byref(blocks))
    assert rc == 1, hip.zfp_hip_last_error().decode()
    assert blocks.value == 0
    assert (words.view(np.uint8) == SENTINEL).all()


def test_host_api_refuses_a_mismatch_in_the_second_pair_and_variable_rate(prod):
    """zfp_compress_regions: the second `in` of another scalar type, extents or
    dimensionality, a shared block and a variable-rate stream return 0, write
    nothing and leave the stream's write position where it was."""
    lib = prod.lib
    lib.zfp_compress_regions.restype = ctypes.c_int
    lib.zfp_compress_regions.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]

    class Chunk(ctypes.Structure):
        _fields_ = [(k, ctypes.c_size_t) for k in ("fx", "fy", "fz", "fw", "ex", "ey", "ez", "ew")]

    words = np.full(4096 * 8, SENTINEL, dtype=np.uint8).view(np.uint64)
    bs = lib.stream_open(words.ctypes.data, words.nbytes)
    zs = lib.zfp_stream_open(bs)
    lib.zfp_stream_set_rate(zs, 8.0, 3, 3, 0)
    lib.zfp_stream_rewind(zs)
    lib.stream_wseek(bs, 96)  # behind a header: 32 bits pending in the bitstream's buffer
    field = lib.zfp_field_3d(None, 3, 16, 12, 8)
    regions = (Chunk * 2)(Chunk(fx=12, fy=8, fz=4, ex=16, ey=12, ez=8),
                          Chunk(fx=2, fy=3, fz=1, ex=10, ey=9, ez=5))  # extents (4, 4, 4) and (8, 6, 4)
    first = np.zeros(4 * 4 * 4, dtype=np.float32)
    src = np.zeros(8 * 6 * 5, dtype=np.float64)

    def call(second_field, regs=regions):
        ifields = (ctypes.c_void_p * 2)(lib.zfp_field_3d(first.ctypes.data, 3, 4, 4, 4), second_field)
        try:
            return lib.zfp_compress_regions(zs, field, None, regs, 2, ifields)
        finally:
            for f in ifields:
                if f:
                    lib.zfp_field_free(f)

    try:
        for ztype, ext in ((4, (8, 6, 4)), (3, (8, 6, 5)), (3, (7, 6, 4))):
            assert call(lib.zfp_field_3d(src.ctypes.data, ztype, *ext)) == 0, (ztype, ext)
        assert call(lib.zfp_field_2d(src.ctypes.data, 3, 8, 6)) == 0, "2D values"
        assert call(None) == 0, "null second field"
        shared = (Chunk * 2)(Chunk(fx=8, fy=8, fz=4, ex=12, ey=12, ez=8), regions[1])  # block (2, 2, 1) twice
        assert call(lib.zfp_field_3d(src.ctypes.data, 3, 8, 6, 4), shared) == 0, "shared block"
        assert lib.zfp_compress_regions(zs, None, None, regions, 2, None) == 0
        assert lib.zfp_compress_regions(zs, field, None, None, 2, None) == 0
        for setter, arg in ((lib.zfp_stream_set_precision, 16), (lib.zfp_stream_set_accuracy, ctypes.c_double(1e-3)),
                            (lib.zfp_stream_set_reversible, None)):
            setter(zs, arg) if arg is not None else setter(zs)
            assert call(lib.zfp_field_3d(src.ctypes.data, 3, 8, 6, 4)) == 0, "variable rate"
        assert lib.stream_wtell(bs) == 96
        assert (words.view(np.uint8) == SENTINEL).all()
    finally:
        lib.zfp_field_free(field)
        lib.zfp_stream_close(zs)
        lib.stream_close(bs)


HOT = "_ZN7zfp_amd13encode3_boxesIfLb0ELi3EEEvNS_9BoxesArgsENS_8GeometryENS_11CodecParamsENS_13RegionEncArgsE"
HOT_VGPRS = 136  # 130 allocated, in the descriptor's granules of 8


def test_batched_encode_kernels_and_their_resources():
    lib = open(LIB_HIP, "rb").read()
    sc = _kernel_scratch(lib)
    boxes = {k: v for k, v in sc.items() if k.startswith("_ZN7zfp_amd13encode3_boxesI")}
    assert len(boxes) == 13, sorted(boxes)  # every type and dimensionality the host can select, double 3D twice
    region = {k: v for k, v in sc.items() if k.startswith("_ZN7zfp_amd14encode3_regionI")}
    assert len(region) == 13, sorted(region)
    assert all(v == 0 for v in boxes.values()), boxes
    assert all(v == 0 for v in region.values()), region
    kd = _descriptor(lib, HOT)
    assert kd is not None and len(kd) == 64, sorted(boxes)
    scratch, = struct.unpack_from("<I", kd, 4)
    rsrc1, = struct.unpack_from("<I", kd, 48)
    vgprs = ((rsrc1 & 0x3f) + 1) * 8
    print("encode3_boxes<float, false, 3>: %d VGPRs (granule 8), %d bytes of scratch" % (vgprs, scratch))
    assert scratch == 0
    assert vgprs == HOT_VGPRS
