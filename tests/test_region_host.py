"""Region decode without a GPU: exports, validation, the hot kernel's scratch.

Every validation failure of zfp_hip_decompress_region / zfp_decompress_region is
decided before any GPU call, returns 0 and leaves the destination untouched, so
these run on a machine without a GPU.  The float 3D lossy region kernel must
keep its plane registers in VGPRs (private segment 0), as decode3<float> does;
the descriptors are read from libzfp_hip.so by kdesc.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from kdesc import _kernel_scratch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "zfp-par_amd", "lib")
LIB_HIP = os.path.join(LIBDIR, "libzfp_hip.so")
LIB_ZFP = os.path.join(LIBDIR, "libzfp.so")
SENTINEL = 0x5A


class Job(ctypes.Structure):
    """zfp_hip_job (include/zfp_hip.h)."""
    _fields_ = [("type", ctypes.c_int32), ("dims", ctypes.c_int32), ("n", ctypes.c_uint64 * 4),
                ("s", ctypes.c_int64 * 4), ("f", ctypes.c_uint64 * 4), ("e", ctypes.c_uint64 * 4),
                ("minbits", ctypes.c_uint32), ("maxbits", ctypes.c_uint32), ("maxprec", ctypes.c_uint32),
                ("minexp", ctypes.c_int32)]


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_libraries_export_the_region_entry_points():
    assert "zfp_decompress_region" in _exports(LIB_ZFP)
    assert "zfp_hip_decompress_region" in _exports(LIB_HIP)


@pytest.fixture(scope="module")
def hip():
    lib = ctypes.CDLL(LIB_HIP)
    lib.zfp_hip_decompress_region.restype = ctypes.c_int
    lib.zfp_hip_decompress_region.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_void_p, ctypes.c_uint64,
                                                                      ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p,
                                                                      ctypes.c_void_p]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


def _job(dims, n, f=None, e=None, ztype=3, rate=8):
    j = Job()
    j.type, j.dims = ztype, dims
    for a in range(dims):
        j.n[a] = n[a]
        j.f[a] = f[a] if f else 0
        j.e[a] = e[a] if e else n[a]
    j.minbits = j.maxbits = rate * 4 ** dims
    j.maxprec, j.minexp = 64, -1074
    return j


def _u64(v):
    return (ctypes.c_uint64 * 4)(*(list(v) + [0] * (4 - len(v))))


def _i64(v):
    return (ctypes.c_int64 * 4)(*(list(v) + [0] * (4 - len(v))))


# (name, job, lo, hi, nulls): what zfp_hip_decompress_region refuses before any GPU call
BOX = dict(f=(4, 0, 8), e=(16, 12, 20))
CASES = [
    ("null job", None, (0, 0, 0), (4, 4, 4), ()),
    ("null lo", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("lo",)),
    ("null hi", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("hi",)),
    ("null dst", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("dst",)),
    ("null strides", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("stride",)),
    ("null words", _job(3, (16, 16, 16)), (0, 0, 0), (4, 4, 4), ("words",)),
    ("empty region", _job(3, (16, 16, 16)), (0, 5, 0), (4, 5, 4), ()),
    ("reversed region", _job(3, (16, 16, 16)), (0, 0, 9), (4, 4, 3), ()),
    ("below the coded box", _job(3, (24, 24, 24), **BOX), (3, 0, 8), (8, 4, 12), ()),
    ("past the coded box", _job(3, (24, 24, 24), **BOX), (4, 0, 8), (8, 4, 21), ()),
    ("past the field", _job(1, (10,)), (2,), (11,), ()),
    ("4D", _job(4, (8, 8, 8, 8)), (0, 0, 0, 0), (4, 4, 4, 4), ()),
]


@pytest.mark.parametrize("name,job,lo,hi,nulls", CASES, ids=[c[0] for c in CASES])
def test_validation_failures_return_0_and_leave_the_destination(hip, name, job, lo, hi, nulls):
    out = np.full(4096, SENTINEL, dtype=np.uint8)
    words = np.zeros(4096, dtype=np.uint64)
    blocks = ctypes.c_uint64(12345)
    rc = hip.zfp_hip_decompress_region(
        ctypes.byref(job) if job is not None else None,
        None if "lo" in nulls else _u64(lo), None if "hi" in nulls else _u64(hi),
        None if "dst" in nulls else out.ctypes.data, None if "stride" in nulls else _i64((1, 4, 16, 64)),
        None if "words" in nulls else words.ctypes.data, len(words), 0, -1, None, ctypes.byref(blocks))
    assert rc == 0, name
    msg = hip.zfp_hip_last_error().decode()
    assert msg and "no HIP device" not in msg, (name, msg)
    if name == "4D":
        assert "4D" in msg, msg
    assert (out == SENTINEL).all(), name
    assert blocks.value == 12345, name


def test_too_many_region_blocks_cannot_be_asked_for(hip):
    """More than 2^32 - 1 region blocks: the coded box itself may hold at most
    2^32 - 1 blocks, so such a region fails with the job (before any GPU call)."""
    out = np.full(64, SENTINEL, dtype=np.uint8)
    words = np.zeros(8, dtype=np.uint64)
    n = (1 << 13, 1 << 13, 1 << 13)  # 2^33 blocks
    rc = hip.zfp_hip_decompress_region(ctypes.byref(_job(3, n)), _u64((0, 0, 0)), _u64(n), out.ctypes.data,
                                       _i64((1, n[0], n[0] * n[1])), words.ctypes.data, len(words), 0, -1, None, None)
    assert rc == 0
    assert "blocks" in hip.zfp_hip_last_error().decode()
    assert (out == SENTINEL).all()


def test_host_api_refuses_type_and_extent_mismatches(prod):
    """zfp_decompress_region: `out` of another scalar type, or of extents that
    are not the region's, returns 0 and writes nothing."""
    lib = prod.lib
    lib.zfp_decompress_region.restype = ctypes.c_int
    lib.zfp_decompress_region.argtypes = [ctypes.c_void_p] * 5

    class Chunk(ctypes.Structure):
        _fields_ = [(k, ctypes.c_size_t) for k in ("fx", "fy", "fz", "fw", "ex", "ey", "ez", "ew")]

    words = np.zeros(4096, dtype=np.uint64)
    bs = lib.stream_open(words.ctypes.data, words.nbytes)
    zs = lib.zfp_stream_open(bs)
    lib.zfp_stream_set_rate(zs, 8.0, 3, 3, 0)
    lib.zfp_stream_rewind(zs)
    field = lib.zfp_field_3d(None, 3, 16, 12, 8)
    region = Chunk(fx=2, fy=3, fz=1, ex=10, ey=9, ez=5)  # extents (8, 6, 4)
    try:
        for ztype, ext in ((4, (8, 6, 4)), (3, (8, 6, 5)), (3, (7, 6, 4))):
            out = np.full(8 * 6 * 5 * 8, SENTINEL, dtype=np.uint8)
            ofield = lib.zfp_field_3d(out.ctypes.data, ztype, *ext)
            assert lib.zfp_decompress_region(zs, field, None, ctypes.byref(region), ofield) == 0, (ztype, ext)
            lib.zfp_field_free(ofield)
            assert (out == SENTINEL).all(), (ztype, ext)
        assert lib.stream_rtell(bs) == 0
    finally:
        lib.zfp_field_free(field)
        lib.zfp_stream_close(zs)
        lib.stream_close(bs)


def test_float_3d_lossy_region_kernel_uses_no_scratch():
    sc = _kernel_scratch(open(LIB_HIP, "rb").read())
    region = {k: v for k, v in sc.items() if k.startswith("_ZN7zfp_amd14decode3_regionI")}
    assert len(region) == 26, sorted(region)  # every type, dimensionality and mode the host can select
    hot = {k: v for k, v in region.items() if re.match(r"_ZN7zfp_amd14decode3_regionIfLb0ELb0ELi3EE", k)}
    assert len(hot) == 1 and all(v == 0 for v in hot.values()), hot
