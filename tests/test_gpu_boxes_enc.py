"""Batched region encode on the GPU (zfp_hip_compress_regions and the layers above it).

Expected streams are the oracle's, never the product's, exactly as
test_gpu_region_encode.py builds them for one region:

  w_old = oracle.compress_words(a)                the stream before the call
  img   = oracle.decompress_words(w_old); img[region] = new   for every region
  w_img = oracle.compress_words(img)
  expected = the start stream with the maxbits-bit field of every block that
             any region touches taken from w_img

(Integer fields take all three steps from the reference library.)  The start
stream is w_old with the bits below bit_offset, every block no region touches
and every covered block overwritten with seeded random bits; only partly
covered blocks keep their valid old bits.  The buffer carries sentinel words on
both sides, and blocks_written must equal the sum of the entries' blocks.
Every case first checks on the CPU that its entries' block sets are pairwise
disjoint.
"""
import ctypes
import zlib

import numpy as np
import pytest

from pyoracle import TYPE_FLOAT, ZFP_MIN_EXP, params_rate
from test_gpu_boxes import Region as DstRegion
from test_gpu_boxes import _dense_aligned, _negative_y, _offset_by_one, _x_stride_2
from test_gpu_region import LIB_HIP, SHAPE, TYPES, _arr4, _blocks, _guarded, _int_field, _job, _special_field
from test_gpu_region_encode import (NSENT, SENT, _bits, _classify, _Codec, _RefCodec, _rate_params, _scramble,
                                    _splice)

pytestmark = pytest.mark.gpu

# numpy axis order (z, y, x); the block sets are pairwise disjoint: 153 blocks, 8 waves
A = ((4, 12), (8, 16), (16, 32))    # 16 blocks, all covered, row loads possible
B = ((12, 20), (0, 8), (3, 30))     # 32 blocks in one wave: 24 covered, 8 cut
C = ((10, 11), (21, 22), (37, 38))  # one element
D = ((17, 21), (22, 26), (60, 72))  # 12 blocks at the field's partial corner: pad rule after overlay
E = ((0, 4), (0, 4), (40, 44))      # with F: stream neighbours that share a word at rate 3.25
F = ((0, 4), (0, 4), (44, 48))
G = ((0, 4), (8, 26), (0, 72))      # 90 blocks: longer than one wave, partial y edge
MAIN = [A, B, C, D, E, F, G]


class SrcRegion(ctypes.Structure):
    """zfp_hip_src_region (include/zfp_hip.h)."""
    _fields_ = [("lo", ctypes.c_uint64 * 4), ("hi", ctypes.c_uint64 * 4), ("src", ctypes.c_void_p),
                ("src_stride", ctypes.c_int64 * 4)]


@pytest.fixture(scope="module")
def hip(product):
    lib = ctypes.CDLL(LIB_HIP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.zfp_hip_compress_regions.restype = ctypes.c_int
    lib.zfp_hip_compress_regions.argtypes = [vp, vp, u64, vp, u64, u64, ctypes.c_int, vp]
    lib.zfp_hip_compress_region.restype = ctypes.c_int
    lib.zfp_hip_compress_region.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, ctypes.c_int, vp]
    lib.zfp_hip_decompress_regions.restype = ctypes.c_int
    lib.zfp_hip_decompress_regions.argtypes = [vp, vp, u64, vp, u64, u64, ctypes.c_int, vp, vp]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


def _table(regions, ptrs, strides, cls=SrcRegion):
    arr = (cls * max(len(regions), 1))()
    for r, region, ptr, st in zip(arr, regions, ptrs, strides):
        r.lo = _arr4(ctypes.c_uint64, [lo for lo, _ in region])
        r.hi = _arr4(ctypes.c_uint64, [hi for _, hi in region])
        setattr(r, "src" if cls is SrcRegion else "dst", ptr)
        setattr(r, "src_stride" if cls is SrcRegion else "dst_stride", _arr4(ctypes.c_int64, st))
    return arr


def _call(hip, job, regions, ptrs, strides, words_ptr, nwords, bit_offset=0):
    blocks = ctypes.c_uint64(12345)
    rc = hip.zfp_hip_compress_regions(ctypes.byref(job), _table(regions, ptrs, strides), len(regions), words_ptr,
                                      nwords, bit_offset, -1, ctypes.byref(blocks))
    return rc, blocks.value


def _classes(codec, regions):
    """Per entry the class of every block (0 missed, 1 cut, 2 covered); the
    entries' block sets must be pairwise disjoint."""
    cls = [_classify(codec.shape, codec.coded, list(r)) for r in regions]
    hits = np.sum([c != 0 for c in cls], axis=0)
    assert hits.max() <= 1, "the test's own entries share a block"
    return cls


def _expect(codec, w_old, regions, news):
    """(w_img, combined class per block) of regions[i] <- news[i] on the stream w_old."""
    cls = _classes(codec, regions)
    img = codec.decompress(w_old).copy()
    for region, new in zip(regions, news):
        img[tuple(slice(lo, hi) for lo, hi in region)] = new
    w_img = codec.compress(img)
    assert len(w_img) == len(w_old)
    return w_img, np.max(cls, axis=0)


def _sources(regions, news, layouts, dtype):
    """Per entry (big, view): the entry's values as the layout's view."""
    out = []
    for k, (region, new) in enumerate(zip(regions, news)):
        lay = layouts[k % len(layouts)] if layouts else _guarded
        big, view = lay([hi - lo for lo, hi in region], dtype)
        view[...] = new
        out.append((big, view))
    return out


def _check(hip, codec, w_old, regions, new, *, seed=0, layouts=None, dev_stream=False, dev_src=False, expect=None):
    """One batch on one stream: the scrambled stream must come back with
    exactly the blocks the entries intersect replaced.  new: a field-sized array
    (every entry takes its own elements of it) or a list of per-entry arrays.
    Returns the valid stream after the update (w_old with those blocks)."""
    regions = [list(r) for r in regions]
    dtype = codec.dtype
    maxbits, off = codec.params[1], codec.bit_offset
    news = new if isinstance(new, list) else [new[tuple(slice(lo, hi) for lo, hi in r)] for r in regions]
    w_img, cls = expect if expect is not None else _expect(codec, w_old, regions, news)
    rng = np.random.default_rng(seed)
    start = _scramble(w_old, cls, maxbits, off, rng)
    touched = np.nonzero(cls)[0]
    want = _splice(start, w_img, touched, maxbits, off)
    buf = np.concatenate([np.full(NSENT, SENT), start, np.full(NSENT, SENT)])
    srcs = _sources(regions, news, layouts, dtype)
    strides = [[s // dtype.itemsize for s in view.strides] for _, view in srcs]
    if dev_stream or dev_src:
        import torch
    keep = []
    if dev_src:
        keep = [torch.from_numpy(big).cuda() for big, _ in srcs]
        ptrs = [d.data_ptr() + (view.ctypes.data - big.ctypes.data) for d, (big, view) in zip(keep, srcs)]
    else:
        ptrs = [view.ctypes.data for _, view in srcs]
    if dev_stream:
        d_buf = torch.from_numpy(buf.view(np.int64)).cuda()
        wptr = d_buf.data_ptr() + 8 * NSENT
    else:
        wptr = buf[NSENT:].ctypes.data
    job = _job(codec.shape, TYPES[dtype], codec.params, codec.coded)
    rc, got = _call(hip, job, regions, ptrs, strides, wptr, len(start), off)
    assert rc == 1, hip.zfp_hip_last_error().decode()
    if dev_stream:
        torch.cuda.synchronize()
        buf = d_buf.cpu().numpy().view(np.uint64)
    assert (buf[:NSENT] == SENT).all() and (buf[-NSENT:] == SENT).all(), "sentinel words written"
    stream = buf[NSENT:NSENT + len(start)]
    bad = np.nonzero(_bits(stream) != _bits(want))[0]
    if bad.size:
        blocks = sorted({int((b - off) // maxbits) for b in bad})
        raise AssertionError(("stream differs in blocks", blocks[:10],
                              [int(cls[b]) if 0 <= b < len(cls) else None for b in blocks[:10]]))
    assert got == len(touched) == sum(_blocks(r, codec.coded, codec.shape) for r in regions), "blocks_written"
    return _splice(w_old, w_img, touched, maxbits, off)


# ---------------------------------------------------------------------------
# the main batch: one oracle pass per (dtype, rate), shared by the tests below
_MAIN_CACHE = {}


def _main(oracle, dtype, rate):
    key = (np.dtype(dtype).name, rate)
    if key not in _MAIN_CACHE:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        a = _special_field(SHAPE, dtype, rng)
        new = _special_field(SHAPE, dtype, rng)
        codec = _Codec(oracle, SHAPE, dtype, _rate_params(rate, dtype, 3))
        w_old = codec.compress(a)
        news = [new[tuple(slice(lo, hi) for lo, hi in r)] for r in MAIN]
        expect = _expect(codec, w_old, MAIN, news)
        for x in (w_old, new, expect[0], expect[1]):
            x.setflags(write=False)
        _MAIN_CACHE[key] = (codec, w_old, new, expect)
    return _MAIN_CACHE[key]


def test_the_main_batch_is_what_it_claims(oracle):
    """Disjoint block sets, 153 blocks in 8 waves, and a wave (B's) with covered
    and read-modify-write lanes."""
    codec = _Codec(oracle, SHAPE, np.float32, _rate_params(16, np.float32, 3))
    cls = _classes(codec, MAIN)
    counts = [int((c != 0).sum()) for c in cls]
    assert counts == [16, 32, 1, 12, 1, 1, 90]
    assert sum(counts) == 153 and sum((n + 63) // 64 for n in counts) == 8
    assert (cls[0][cls[0] != 0] == 2).all()
    assert int((cls[1] == 2).sum()) == 24 and int((cls[1] == 1).sum()) == 8 and counts[1] <= 64
    assert int((cls[3] == 1).sum()) > 0  # D is cut at its low z and y sides and padded at the field's corner
    # E and F are neighbours in the stream
    e, f = int(np.nonzero(cls[4])[0][0]), int(np.nonzero(cls[5])[0][0])
    assert f == e + 1 and ((e + 1) * 208) % 64 != 0


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rate", [16, 8, 5, 3.25])
def test_main_batch_matches_oracle(hip, oracle, dtype, rate, order):
    codec, w_old, new, expect = _main(oracle, dtype, rate)
    assert codec.params[1] == {16: 1024, 8: 512, 5: 320, 3.25: 208}[rate]
    regions = MAIN if order == "forward" else MAIN[::-1]
    _check(hip, codec, w_old, regions, new, expect=expect, seed=1)


@pytest.mark.parametrize("dev_src", [False, True], ids=["host sources", "device sources"])
def test_layouts_differ_per_region(hip, oracle, dev_src):
    """Dense and aligned (A: 16-byte rows from a device source), offset by one
    element, x stride 2, negative y stride, and so on round the entries."""
    codec, w_old, new, expect = _main(oracle, np.float32, 8)
    _check(hip, codec, w_old, MAIN, new, expect=expect, seed=2, dev_src=dev_src, dev_stream=dev_src,
           layouts=[_dense_aligned, _offset_by_one, _x_stride_2, _negative_y])


# ---- many entries, one entry ----
def test_seventy_single_elements(hip, oracle):
    """70 entries of one element in 70 distinct blocks: 70 waves, bisection depth 7."""
    codec, w_old, new, _ = _main(oracle, np.float32, 8)
    rng = np.random.default_rng(70)
    nb = [(n + 3) // 4 for n in SHAPE]
    regions = []
    for b in rng.choice(int(np.prod(nb)), size=70, replace=False):
        bi = np.unravel_index(int(b), nb)
        c = [min(4 * int(i) + int(rng.integers(0, 4)), n - 1) for i, n in zip(bi, SHAPE)]
        regions.append(tuple((x, x + 1) for x in c))
    _check(hip, codec, w_old, regions, new, seed=3)


@pytest.mark.parametrize("rate", [16, 3.25])
def test_one_entry_the_whole_field(hip, oracle, rate):
    """Every block covered: the result is the oracle's stream of the new field."""
    codec, w_old, new, _ = _main(oracle, np.float32, rate)
    whole = [tuple((0, n) for n in SHAPE)]
    got = _check(hip, codec, w_old, whole, new, seed=4)
    assert got.tobytes() == codec.compress(new).tobytes()


# ---- rows crossing waves and workgroups ----
@pytest.mark.parametrize("dtype,params", [(np.float32, params_rate(12, TYPE_FLOAT, 3)),
                                          (np.float64, (768, 768, 32, ZFP_MIN_EXP))])
def test_long_rows_cross_waves_and_workgroups(hip, oracle, dtype, params):
    """3 x 3 x 75 blocks.  The first entry has 300 blocks (5 waves: it crosses
    into the second workgroup), the second starts in wave 1 of that workgroup,
    the third in wave 2; f64 with maxprec 32 is the planes-32..63 coder."""
    shape = (9, 9, 300)
    rng = np.random.default_rng(5)
    a = _special_field(shape, dtype, rng)
    new = _special_field(shape, dtype, rng)
    codec = _Codec(oracle, shape, dtype, params)
    w_old = codec.compress(a)
    regions = [((0, 8), (0, 8), (2, 299)), ((8, 9), (1, 9), (250, 300)), ((1, 7), (8, 9), (0, 300))]
    assert [_blocks(list(r), None, shape) for r in regions] == [300, 39, 150]
    _check(hip, codec, w_old, regions, new, seed=5)


# ---- header offset, coded chunk ----
def test_stream_behind_a_header(hip, oracle):
    """Blocks start at bit 96: the 96 bits below stay, every block straddles words."""
    shape = (20, 24, 36)
    rng = np.random.default_rng(11)
    a = rng.standard_normal(shape).astype(np.float32)
    new = rng.standard_normal(shape).astype(np.float32)
    codec = _Codec(oracle, shape, np.float32, params_rate(8, 0, 3), bit_offset=96)
    w_old = codec.compress(a)
    _check(hip, codec, w_old, [((1, 12), (3, 23), (5, 34)), ((12, 20), (0, 24), (0, 4)), ((13, 14), (7, 8), (4, 36))],
           new, seed=6)


def test_coded_chunk_inside_a_larger_field(hip, oracle):
    """Blocks count from the chunk's origin (8, 4, 12)."""
    shape = (24, 24, 48)
    coded = [(8, 20), (4, 24), (12, 40)]
    rng = np.random.default_rng(3)
    a = _special_field(shape, np.float32, rng)
    new = _special_field(shape, np.float32, rng)
    codec = _Codec(oracle, shape, np.float32, params_rate(8, TYPE_FLOAT, 3), coded=coded)
    w_old = codec.compress(a)
    _check(hip, codec, w_old, [((8, 13), (4, 11), (12, 30)),     # low corner at the box's f
                               ((16, 20), (9, 22), (17, 39)),    # the box's last z blocks
                               ((9, 16), (12, 24), (12, 40))],   # beside the first, up to the box's e
           new, seed=7)


# ---- 1D / 2D, integers ----
R1 = [((3, 20),), ((20, 40),), ((66, 70),)]
R2 = [((2, 11), (5, 16)), ((0, 13), (16, 34)), ((12, 13), (0, 4))]


@pytest.mark.parametrize("rate", [8, 3.25])
@pytest.mark.parametrize("dtype,shape,regions", [(np.float32, (13, 37), R2), (np.float64, (70,), R1)])
def test_1d_2d_floats_match_oracle(hip, oracle, dtype, shape, regions, rate):
    rng = np.random.default_rng(29)
    a = (rng.standard_normal(shape) * 100).astype(dtype)
    new = (rng.standard_normal(shape) * 100).astype(dtype)
    codec = _Codec(oracle, shape, dtype, _rate_params(rate, dtype, len(shape)))
    w_old = codec.compress(a)
    _check(hip, codec, w_old, regions, new, seed=8)
    _check(hip, codec, w_old, regions[::-1][:2], new, seed=9)


@pytest.mark.parametrize("dtype,shape,regions", [(np.int32, (70,), R1), (np.int32, (13, 37), R2),
                                                 (np.int32, SHAPE, MAIN), (np.int64, (13, 37), R2)],
                         ids=["int32-1d", "int32-2d", "int32-3d", "int64-2d"])
def test_integers_match_reference(hip, ref_capi, dtype, shape, regions):
    a = _int_field(shape, dtype, 31)
    new = _int_field(shape, dtype, 37)
    codec = _RefCodec(ref_capi, shape, dtype, 8)
    w_old = codec.compress(a)
    _check(hip, codec, w_old, regions, new, seed=10)


# ---- memory kinds ----
@pytest.mark.parametrize("dev_stream,dev_src", [(False, False), (True, True), (True, False)],
                         ids=["host-host", "device-device", "device stream-host sources"])
def test_host_and_device_memory(hip, oracle, dev_stream, dev_src):
    codec, w_old, new, expect = _main(oracle, np.float32, 3.25)
    _check(hip, codec, w_old, MAIN, new, expect=expect, seed=12, dev_stream=dev_stream, dev_src=dev_src)


def test_mixed_sources_are_refused(hip, oracle):
    import torch
    codec, w_old, new, _ = _main(oracle, np.float32, 16)
    job = _job(SHAPE, TYPE_FLOAT, codec.params)
    regions = [list(A), list(E), list(F)]
    host = [np.ascontiguousarray(new[tuple(slice(lo, hi) for lo, hi in r)]) for r in regions]
    dev = torch.from_numpy(host[1]).cuda()
    d_words = torch.from_numpy(w_old.view(np.int64).copy()).cuda()
    ptrs = [host[0].ctypes.data, dev.data_ptr(), host[2].ctypes.data]
    strides = [[s // 4 for s in h.strides] for h in host]
    rc, blocks = _call(hip, job, regions, ptrs, strides, d_words.data_ptr(), len(w_old))
    assert rc == 0 and blocks == 12345
    assert "regions[1]" in hip.zfp_hip_last_error().decode()
    torch.cuda.synchronize()
    assert d_words.cpu().numpy().view(np.uint64).tobytes() == w_old.tobytes()


# ---- batch equals loop (secondary to the oracle comparison above) ----
@pytest.mark.parametrize("rate", [8, 3.25])
def test_batch_equals_a_loop_of_single_calls(hip, oracle, rate):
    codec, w_old, new, (w_img, cls) = _main(oracle, np.float32, rate)
    start = _scramble(w_old, cls, codec.params[1], 0, np.random.default_rng(13))
    job = _job(SHAPE, TYPE_FLOAT, codec.params)
    srcs = [np.ascontiguousarray(new[tuple(slice(lo, hi) for lo, hi in r)]) for r in MAIN]
    strides = [[s // 4 for s in s_.strides] for s_ in srcs]
    batch = start.copy()
    rc, nb = _call(hip, job, MAIN, [s.ctypes.data for s in srcs], strides, batch.ctypes.data, len(batch))
    assert rc == 1, hip.zfp_hip_last_error().decode()
    loop = start.copy()
    total = 0
    for r, s, st in zip(MAIN, srcs, strides):
        blocks = ctypes.c_uint64(0)
        rc = hip.zfp_hip_compress_region(ctypes.byref(job), _arr4(ctypes.c_uint64, [lo for lo, _ in r]),
                                         _arr4(ctypes.c_uint64, [hi for _, hi in r]), s.ctypes.data,
                                         _arr4(ctypes.c_int64, st), loop.ctypes.data, len(loop), 0, -1,
                                         ctypes.byref(blocks))
        assert rc == 1, hip.zfp_hip_last_error().decode()
        total += blocks.value
    assert batch.tobytes() == loop.tobytes() and nb == total == 153


# ---- one context, call after call ----
def test_context_reuse_across_batches(hip, oracle):
    """On one thread every call gets the same context back: the table, the
    field scratch and the staging are handed on.  Batched encode, batched decode
    of the same regions, a single region encode, a batch with fewer entries, a
    refused (overlapping) batch, a batch with more entries."""
    codec, w_old, new, expect = _main(oracle, np.float32, 5)
    rng = np.random.default_rng(17)
    job = _job(SHAPE, TYPE_FLOAT, codec.params)
    cur = _check(hip, codec, w_old, MAIN, new, expect=expect, seed=14)
    # batched decode of the same regions from the updated stream
    ref = codec.decompress(cur)
    outs = [np.full([hi - lo for lo, hi in r], 7.0, dtype=np.float32) for r in MAIN]
    blocks = ctypes.c_uint64(0)
    table = _table(MAIN, [o.ctypes.data for o in outs], [[s // 4 for s in o.strides] for o in outs], DstRegion)
    assert hip.zfp_hip_decompress_regions(ctypes.byref(job), table, len(MAIN), cur.ctypes.data, len(cur), 0, -1, None,
                                          ctypes.byref(blocks)) == 1, hip.zfp_hip_last_error().decode()
    assert blocks.value == 153
    for r, o in zip(MAIN, outs):
        assert o.tobytes() == np.ascontiguousarray(ref[tuple(slice(lo, hi) for lo, hi in r)]).tobytes(), r
    # a single region encode through the same context
    new2 = _special_field(SHAPE, np.float32, rng)
    one = [(3, 19), (5, 22), (6, 70)]
    part = np.ascontiguousarray(new2[tuple(slice(lo, hi) for lo, hi in one)])
    w_img, cls = _expect(codec, cur, [one], [part])
    w = cur.copy()
    assert hip.zfp_hip_compress_region(ctypes.byref(job), _arr4(ctypes.c_uint64, [lo for lo, _ in one]),
                                       _arr4(ctypes.c_uint64, [hi for _, hi in one]), part.ctypes.data,
                                       _arr4(ctypes.c_int64, [s // 4 for s in part.strides]), w.ctypes.data, len(w), 0,
                                       -1, None) == 1, hip.zfp_hip_last_error().decode()
    cur = _splice(cur, w_img, np.nonzero(cls)[0], codec.params[1], 0)
    assert w.tobytes() == cur.tobytes()
    # fewer entries
    new3 = _special_field(SHAPE, np.float32, rng)
    cur = _check(hip, codec, cur, [B, G], new3, seed=15)
    # a refused batch: C lies in a block of the first entry; the stream stays
    w = cur.copy()
    regs = [list(r) for r in (((8, 12), (20, 24), (36, 40)), A, C)]
    srcs = [np.ascontiguousarray(new3[tuple(slice(lo, hi) for lo, hi in r)]) for r in regs]
    rc, nb = _call(hip, job, regs, [s.ctypes.data for s in srcs], [[x // 4 for x in s.strides] for s in srcs],
                   w.ctypes.data, len(w))
    msg = hip.zfp_hip_last_error().decode()
    assert rc == 0 and nb == 12345 and "regions[0]" in msg and "regions[2]" in msg, msg
    assert w.tobytes() == cur.tobytes()
    # more entries than any call before
    regions = MAIN + [((12, 20), (8, 20), (32, 60)), ((20, 21), (0, 4), (0, 8)), ((4, 8), (0, 8), (0, 16))]
    new4 = _special_field(SHAPE, np.float32, rng)
    cur = _check(hip, codec, cur, regions, new4, seed=16)
    assert cur.tobytes() != w_old.tobytes()


# ---------------------------------------------------------------------------
# zfpy
def test_zfpy_compress_regions(oracle):
    import zfpy
    rng = np.random.default_rng(41)
    a = rng.standard_normal(SHAPE).astype(np.float32)
    new = rng.standard_normal(SHAPE).astype(np.float32)
    s0 = zfpy.compress_numpy(a, rate=8)
    hbits = 96
    params = params_rate(8, 0, 3)
    codec = _Codec(oracle, SHAPE, np.float32, params, bit_offset=hbits)
    w_old = np.frombuffer(s0, dtype=np.uint64).copy()
    regions = [tuple(slice(lo, hi) for lo, hi in r) for r in MAIN]
    news = [new[r] for r in regions]  # strided views of the field
    w_img, cls = _expect(codec, w_old, MAIN, news)
    want = _splice(w_old, w_img, np.nonzero(cls)[0], params[1], hbits)
    s = bytearray(s0)
    assert zfpy.compress_regions(s, regions, news) == 153
    assert bytes(s) == want.tobytes()
    got = zfpy.decompress_regions(s, regions)
    ref = codec.decompress(want)
    for g, r in zip(got, regions):
        assert g.tobytes() == np.ascontiguousarray(ref[r]).tobytes(), r
    # the rows of an (N, d, h, w) array
    corners = [(0, 0, 0), (12, 16, 28), (4, 8, 12), (8, 8, 48)]
    crops = [tuple(slice(c, c + 8) for c in corner) for corner in corners]
    boxes = [[(c, c + 8) for c in corner] for corner in corners]
    stack = rng.standard_normal((4, 8, 8, 8)).astype(np.float32)
    w_img, cls = _expect(codec, w_old, boxes, list(stack))
    t = np.frombuffer(bytearray(s0), dtype=np.uint8)
    assert zfpy.compress_regions(t, crops, stack) == 32
    assert bytes(t) == _splice(w_old, w_img, np.nonzero(cls)[0], params[1], hbits).tobytes()
    assert zfpy.compress_regions(bytearray(s0), [], []) == 0
    with pytest.raises(TypeError):
        zfpy.compress_regions(bytes(s0), regions, news)
    with pytest.raises(ValueError):
        zfpy.compress_regions(bytearray(zfpy.compress_numpy(a, precision=16)), regions, news)
    before = bytes(s)
    with pytest.raises(TypeError):
        zfpy.compress_regions(s, regions, news[:-1] + [news[-1].astype(np.float64)])
    with pytest.raises(ValueError):
        zfpy.compress_regions(s, regions, news[:-1] + [news[-1][:, :, :60]])
    with pytest.raises(ValueError):
        zfpy.compress_regions(s, regions, news[:-1])
    # elements disjoint from C's one, C's block shared
    with pytest.raises(ValueError, match=r"regions\[2\].*regions\[7\]"):
        zfpy.compress_regions(s, regions + [(slice(8, 12), slice(20, 24), slice(38, 40))],
                              news + [np.zeros((4, 4, 2), dtype=np.float32)])
    assert bytes(s) == before


# zfp_parallel
def test_zfp_parallel_compress_regions(oracle):
    import zfpy
    shape = (64, 64, 96)
    rng = np.random.default_rng(43)
    idx = np.indices(shape, dtype=np.float32)
    a = (np.sin(0.05 * idx[0]) + np.cos(0.07 * idx[1]) * np.sin(0.03 * idx[2])
         + 1e-3 * rng.standard_normal(shape)).astype(np.float32)
    zps = []
    for _ in range(2):
        zp = zfpy.zfp_parallel(shape, "float32", nparts=8)
        zp.get_numpy_array()[...] = a
        zp.compress(nthreads=8, rate=8)
        zps.append(zp)
    zp, zq = zps
    boxes = zp.get_chunkit().boxes
    assert len(boxes) == 8
    x, y, z = boxes[3][:3]  # one chunk's box (x first)
    inside = (slice(z[0] + 1, z[1] - 1), slice(y[0] + 2, y[1] - 1), slice(x[0] + 3, x[0] + 9))
    # three regions that straddle chunks and one strictly inside chunk 3, block sets disjoint within every chunk
    regions = [(slice(5, 61), slice(3, 62), slice(16, 40)), (slice(0, 64), slice(0, 64), slice(44, 47)),
               (slice(30, 34), slice(30, 34), slice(88, 96))]
    news = [rng.standard_normal([s.stop - s.start for s in r]).astype(np.float32) for r in regions]
    before = list(zp._compress_data)
    out = zp.compress_regions(regions, news, nthreads=8)
    assert out is zp._compress_data and all(isinstance(s, bytes) for s in out)
    for r, v in zip(regions, news):
        zq.compress_region(r, v, nthreads=8)
    assert list(out) == list(zq._compress_data)
    coded = [list(reversed(b[:3])) for b in boxes]  # numpy axis order
    hit = [any(all(max(s.start, cf) < min(s.stop, ce) for s, (cf, ce) in zip(r, cd)) for r in regions) for cd in coded]
    assert hit[0] and [o is not b for o, b in zip(out, before)] == hit
    # the oracle's word on one chunk: chunk 0's parts of the three regions
    codec = _Codec(oracle, shape, np.float32, params_rate(8, 0, 3), coded=[tuple(c) for c in coded[0]], bit_offset=96)
    parts, subs = [], []
    for r, v in zip(regions, news):
        box = [(s.start, s.stop) for s in r]
        part = [(max(f, cf), min(e, ce)) for (f, e), (cf, ce) in zip(box, coded[0])]
        if all(f < e for f, e in part):
            parts.append(part)
            subs.append(v[tuple(slice(f - f0, e - f0) for (f, e), (f0, _) in zip(part, box))])
    assert len(parts) >= 2
    w0 = np.frombuffer(before[0], dtype=np.uint64).copy()
    w_img, cls = _expect(codec, w0, parts, subs)
    assert out[0] == _splice(w0, w_img, np.nonzero(cls)[0], 512, 96).tobytes()
    # one region inside chunk 3, values from the shared array: the other chunks keep their objects
    new2 = rng.standard_normal(shape).astype(np.float32)
    for p in (zp, zq):
        p.get_numpy_array()[...] = new2
    before = list(zp._compress_data)
    zp.compress_regions([inside], nthreads=8)
    zq.compress_region(inside, nthreads=8)
    for i in range(8):
        assert zp._compress_data[i] == zq._compress_data[i], i
        assert (zp._compress_data[i] is before[i]) == (i != 3), i
    # parts that share a block within a chunk: nothing is touched
    before = list(zp._compress_data)
    with pytest.raises(ValueError):
        zp.compress_regions([(slice(0, 64), slice(0, 64), slice(0, 6)), (slice(0, 64), slice(0, 64), slice(6, 20))])
    assert all(s is b for s, b in zip(zp._compress_data, before))
    zp.compress(nthreads=8, precision=16)
    with pytest.raises(RuntimeError):
        zp.compress_regions([inside])
