"""Region encode without a GPU: exports and validation.

Every validation failure of zfp_hip_compress_region / zfp_compress_region is
decided before any GPU call, returns 0 and leaves the stream untouched, so
these run on a machine without a GPU.
"""
import ctypes
import os

import numpy as np
import pytest

from test_region_host import BOX, _exports, _i64, _job, _u64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "zfp-par_amd", "lib")
LIB_HIP = os.path.join(LIBDIR, "libzfp_hip.so")
LIB_ZFP = os.path.join(LIBDIR, "libzfp.so")
SENTINEL = 0x5A


def test_libraries_export_the_region_encode_entry_points():
    assert "zfp_compress_region" in _exports(LIB_ZFP)
    assert "zfp_hip_compress_region" in _exports(LIB_HIP)


@pytest.fixture(scope="module")
def hip():
    lib = ctypes.CDLL(LIB_HIP)
    lib.zfp_hip_compress_region.restype = ctypes.c_int
    lib.zfp_hip_compress_region.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_void_p, ctypes.c_uint64,
                                                                    ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


def _variable(job, minbits=1, maxbits=16658, maxprec=20, minexp=-1074):
    job.minbits, job.maxbits, job.maxprec, job.minexp = minbits, maxbits, maxprec, minexp
    return job


# (name, job, lo, hi, nulls, capacity words or None for the whole buffer)
CASES = [
    ("null job", None, (0, 0, 0), (4, 4, 4), (), None),
    ("null lo", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("lo",), None),
    ("null hi", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("hi",), None),
    ("null src", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("src",), None),
    ("null strides", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("stride",), None),
    ("null words", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("words",), None),
    ("empty region", _job(3, (16, 16, 16)), (0, 5, 0), (4, 5, 4), (), None),
    ("reversed region", _job(3, (16, 16, 16)), (0, 0, 9), (4, 4, 3), (), None),
    ("below the coded box", _job(3, (24, 24, 24), **BOX), (3, 0, 8), (8, 4, 12), (), None),
    ("past the coded box", _job(3, (24, 24, 24), **BOX), (4, 0, 8), (8, 4, 21), (), None),
    ("past the field", _job(1, (10,)), (2,), (11,), (), None),
    ("4D", _job(4, (8, 8, 8, 8)), (0, 0, 0, 0), (4, 4, 4, 4), (), None),
    ("variable rate: precision", _variable(_job(3, (16, 16, 16))), (0, 0, 0), (4, 4, 4), (), None),
    ("variable rate: accuracy", _variable(_job(3, (16, 16, 16)), maxprec=64, minexp=-10), (0, 0, 0), (4, 4, 4), (),
     None),
    ("variable rate: reversible", _variable(_job(3, (16, 16, 16)), maxprec=64, minexp=-1075), (0, 0, 0), (4, 4, 4),
     (), None),
    ("variable rate: minbits < maxbits", _variable(_job(3, (16, 16, 16)), 256, 512, 64), (0, 0, 0), (4, 4, 4), (),
     None),
    # 16^3 at rate 8: 64 blocks of 8 words; the last block of [8:16, 8:16, 8:16] is block 63
    ("stream ends before the last needed block", _job(3, (16, 16, 16)), (8, 8, 8), (16, 16, 16), (), 511),
    ("stream ends inside the first block", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), (), 7),
    ("empty stream", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), (), 0),
]


@pytest.mark.parametrize("name,job,lo,hi,nulls,cap", CASES, ids=[c[0] for c in CASES])
def test_validation_failures_return_0_and_leave_the_stream(hip, name, job, lo, hi, nulls, cap):
    src = np.zeros(4096, dtype=np.float32)
    words = np.full(4096, SENTINEL, dtype=np.uint8).view(np.uint64)
    blocks = ctypes.c_uint64(12345)
    rc = hip.zfp_hip_compress_region(
        ctypes.byref(job) if job is not None else None,
        None if "lo" in nulls else _u64(lo), None if "hi" in nulls else _u64(hi),
        None if "src" in nulls else src.ctypes.data, None if "stride" in nulls else _i64((1, 4, 16, 64)),
        None if "words" in nulls else words.ctypes.data, len(words) if cap is None else cap, 0, -1,
        ctypes.byref(blocks))
    assert rc == 0, name
    msg = hip.zfp_hip_last_error().decode()
    assert msg and "no HIP device" not in msg, (name, msg)
    if name == "4D":
        assert "4D" in msg, msg
    if name.startswith("variable rate"):
        assert "fixed-rate" in msg, msg
    assert (words.view(np.uint8) == SENTINEL).all(), name
    assert blocks.value == 12345, name


def test_a_bit_offset_counts_towards_the_capacity(hip):
    """64 blocks of 512 bits behind 96 header bits need 514 words, not 512."""
    job = _job(3, (16, 16, 16))
    src = np.zeros(4096, dtype=np.float32)
    words = np.full(514 * 8, SENTINEL, dtype=np.uint8).view(np.uint64)
    rc = hip.zfp_hip_compress_region(ctypes.byref(job), _u64((0, 0, 0)), _u64((16, 16, 16)), src.ctypes.data,
                                     _i64((1, 16, 256)), words.ctypes.data, 513, 96, -1, None)
    assert rc == 0
    msg = hip.zfp_hip_last_error().decode()
    assert msg and "no HIP device" not in msg, msg
    assert (words.view(np.uint8) == SENTINEL).all()


def test_too_many_region_blocks_cannot_be_asked_for(hip):
    """More than 2^32 - 1 region blocks: the coded box itself may hold at most
    2^32 - 1 blocks, so such a region fails with the job (before any GPU call)."""
    src = np.zeros(64, dtype=np.float32)
    words = np.full(8, SENTINEL, dtype=np.uint8).view(np.uint64)
    n = (1 << 13, 1 << 13, 1 << 13)  # 2^33 blocks
    rc = hip.zfp_hip_compress_region(ctypes.byref(_job(3, n)), _u64((0, 0, 0)), _u64(n), src.ctypes.data,
                                     _i64((1, n[0], n[0] * n[1])), words.ctypes.data, len(words), 0, -1, None)
    assert rc == 0
    assert "blocks" in hip.zfp_hip_last_error().decode()
    assert (words.view(np.uint8) == SENTINEL).all()


def test_host_api_refuses_mismatches_and_variable_rate(prod):
    """zfp_compress_region: `in` of another scalar type, dimensionality or of
    extents that are not the region's, and a variable-rate stream, return 0,
    write nothing and leave the stream's write position where it was."""
    lib = prod.lib
    lib.zfp_compress_region.restype = ctypes.c_int
    lib.zfp_compress_region.argtypes = [ctypes.c_void_p] * 5

    class Chunk(ctypes.Structure):
        _fields_ = [(k, ctypes.c_size_t) for k in ("fx", "fy", "fz", "fw", "ex", "ey", "ez", "ew")]

    words = np.full(4096 * 8, SENTINEL, dtype=np.uint8).view(np.uint64)
    bs = lib.stream_open(words.ctypes.data, words.nbytes)
    zs = lib.zfp_stream_open(bs)
    lib.zfp_stream_set_rate(zs, 8.0, 3, 3, 0)
    lib.zfp_stream_rewind(zs)
    lib.stream_wseek(bs, 96)  # behind a header: 32 bits pending in the bitstream's buffer
    field = lib.zfp_field_3d(None, 3, 16, 12, 8)
    region = Chunk(fx=2, fy=3, fz=1, ex=10, ey=9, ez=5)  # extents (8, 6, 4)
    src = np.zeros(8 * 6 * 5, dtype=np.float64)
    try:
        for ztype, ext in ((4, (8, 6, 4)), (3, (8, 6, 5)), (3, (7, 6, 4))):
            ifield = lib.zfp_field_3d(src.ctypes.data, ztype, *ext)
            assert lib.zfp_compress_region(zs, field, None, ctypes.byref(region), ifield) == 0, (ztype, ext)
            lib.zfp_field_free(ifield)
        ifield = lib.zfp_field_2d(src.ctypes.data, 3, 8, 6)
        assert lib.zfp_compress_region(zs, field, None, ctypes.byref(region), ifield) == 0, "2D values"
        lib.zfp_field_free(ifield)
        ifield = lib.zfp_field_3d(src.ctypes.data, 3, 8, 6, 4)
        assert lib.zfp_compress_region(zs, None, None, ctypes.byref(region), ifield) == 0
        assert lib.zfp_compress_region(zs, field, None, None, ifield) == 0
        assert lib.zfp_compress_region(zs, field, None, ctypes.byref(region), None) == 0
        lib.zfp_stream_set_precision(zs, 16)
        assert lib.zfp_compress_region(zs, field, None, ctypes.byref(region), ifield) == 0, "variable rate"
        lib.zfp_stream_set_accuracy(zs, 1e-3)
        assert lib.zfp_compress_region(zs, field, None, ctypes.byref(region), ifield) == 0, "variable rate"
        lib.zfp_stream_set_reversible(zs)
        assert lib.zfp_compress_region(zs, field, None, ctypes.byref(region), ifield) == 0, "variable rate"
        lib.zfp_field_free(ifield)
        assert lib.stream_wtell(bs) == 96
        assert (words.view(np.uint8) == SENTINEL).all()
    finally:
        lib.zfp_field_free(field)
        lib.zfp_stream_close(zs)
        lib.stream_close(bs)
