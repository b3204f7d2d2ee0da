"""Region encode on the GPU (zfp_hip_compress_region and the layers above it).

Expected streams are the oracle's, never the product's:

  w_old = oracle.compress_words(a)                the stream before the call
  img   = oracle.decompress_words(w_old); img[region] = new
  w_img = oracle.compress_words(img)
  expected = w_old with the maxbits-bit field of every block that intersects
             the region taken from w_img

(Integer fields, which the oracle does not code, take all three steps from the
reference library as test_gpu_types.py does.)

Re-encoding decoded data reproduces most blocks bit for bit, so a plain
comparison would not notice an implementation that rewrites too much.  Before
the call the old bits of every block the call must not read -- every block that
does not intersect the region and every covered block -- are overwritten with
seeded random bits: the non-intersecting ones must come back unchanged, the
covered ones equal to w_img's.  Only partly covered blocks keep their valid old
bits.  The stream buffer carries sentinel words before word 0 and after the
last word, and blocks_written must equal the number of intersecting blocks.
"""
import ctypes
import itertools
import os
import zlib

import numpy as np
import pytest

from pyoracle import TYPE_FLOAT, ZFP_MIN_EXP, params_rate

from test_gpu_region import (REGIONS, SHAPE, TYPES, _arr4, _blocks, _guarded, _int_field, _job, _special_field,
                             _strided_views)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_HIP = os.path.join(REPO, "zfp-par_amd", "lib", "libzfp_hip.so")
SENT = np.uint64(0xA5A5A5A55A5A5A5A)
NSENT = 3


@pytest.fixture(scope="module")
def hip(product):
    lib = ctypes.CDLL(LIB_HIP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.zfp_hip_compress_region.restype = ctypes.c_int
    lib.zfp_hip_compress_region.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, ctypes.c_int, vp]
    lib.zfp_hip_decompress.restype = ctypes.c_int
    lib.zfp_hip_decompress.argtypes = [vp, vp, vp, u64, u64, ctypes.c_int, vp, vp]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


# ---------------------------------------------------------------------------
# bit-level helpers (numpy axis order throughout; block raster order: x, the
# last numpy axis, fastest)
def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")


def _words(bits):
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def _norm(region, shape):
    return [(0 if r is None else r[0], n if r is None else r[1]) for r, n in zip(region, shape)]


def _classify(shape, coded, region):
    """Per block of the coded box, in stream order: 0 the region misses it, 1 it
    cuts through it (or the block codes elements past the box), 2 covered
    (every element of the block inside the field is inside the region)."""
    coded = coded or [(0, n) for n in shape]
    nb = [(e - f + 3) // 4 for f, e in coded]
    out = np.zeros(nb, dtype=np.int8)
    for bi in itertools.product(*(range(n) for n in nb)):
        hit, cov = True, True
        for a, i in enumerate(bi):
            b0 = coded[a][0] + 4 * i
            b1 = min(b0 + 4, shape[a])  # the block's elements inside the field
            lo, hi = region[a]
            hit = hit and lo < b1 and b0 < hi
            cov = cov and lo <= b0 and b1 <= hi
        out[bi] = 2 if hit and cov else 1 if hit else 0
    return out.reshape(-1)


def _splice(base_words, from_words, which, maxbits, bit_offset):
    """base_words with the maxbits-bit field of every block in `which` (stream
    block numbers) taken from from_words."""
    bits = _bits(base_words)
    src = _bits(from_words)
    for B in which:
        p = bit_offset + int(B) * maxbits
        bits[p:p + maxbits] = src[p:p + maxbits]
    return _words(bits)


def _scramble(words, cls, maxbits, bit_offset, rng):
    """Random bits below bit_offset and in every block the call must not read."""
    bits = _bits(words)
    bits[:bit_offset] = rng.integers(0, 2, size=bit_offset, dtype=np.uint8)
    for B in np.nonzero(cls != 1)[0]:
        p = bit_offset + int(B) * maxbits
        bits[p:p + maxbits] = rng.integers(0, 2, size=maxbits, dtype=np.uint8)
    return _words(bits)


class _Codec:
    """compress(arr) -> words, decompress(words) -> arr for one stream layout."""

    def __init__(self, oracle, shape, dtype, params, coded=None, bit_offset=0):
        self.shape, self.dtype, self.params, self.coded, self.bit_offset = shape, np.dtype(dtype), params, coded, bit_offset
        self.box = (list(reversed(coded)) + [(0, 0)] * (4 - len(coded))) if coded else None
        self.o = oracle

    def compress(self, a):
        return self.o.compress_words(np.ascontiguousarray(a), self.params, box=self.box, bit_offset=self.bit_offset)[0]

    def decompress(self, w):
        return self.o.decompress_words(w, self.shape, self.dtype, self.params, box=self.box,
                                       bit_offset=self.bit_offset)[0]


class _RefCodec:
    """The same through the reference library (integer fields)."""

    def __init__(self, ref, shape, dtype, rate):
        self.shape, self.dtype, self.rate, self.ref = shape, np.dtype(dtype), rate, ref
        self.ztype = TYPES[self.dtype]
        self.params = params_rate(rate, self.ztype, len(shape))
        self.coded, self.bit_offset = None, 0

    def compress(self, a):
        data = self.ref.compress(np.ascontiguousarray(a), "rate", self.rate, ztype=self.ztype)
        return np.frombuffer(data + bytes((-len(data)) % 8), dtype=np.uint64).copy()

    def decompress(self, w):
        return self.ref.decompress(w.tobytes(), self.shape, self.dtype, "rate", self.rate, ztype=self.ztype)[0]


def _expect(codec, w_old, region, new):
    """(expected words, class per block) of `region` <- `new` on the stream w_old."""
    img = codec.decompress(w_old).copy()
    img[tuple(slice(lo, hi) for lo, hi in region)] = new
    w_img = codec.compress(img)
    assert len(w_img) == len(w_old)
    cls = _classify(codec.shape, codec.coded, region)
    return w_img, cls


def _call(hip, job, region, src_ptr, src_strides, words_ptr, nwords, bit_offset):
    blocks = ctypes.c_uint64(0)
    rc = hip.zfp_hip_compress_region(ctypes.byref(job), _arr4(ctypes.c_uint64, [lo for lo, _ in region]),
                                     _arr4(ctypes.c_uint64, [hi for _, hi in region]), src_ptr,
                                     _arr4(ctypes.c_int64, src_strides), words_ptr, nwords, bit_offset, -1,
                                     ctypes.byref(blocks))
    assert rc == 1, hip.zfp_hip_last_error().decode()
    return blocks.value


def _strided_source(new):
    """`new` as a strided view inside a larger array."""
    big, view = _guarded(list(new.shape), new.dtype)
    view[...] = new
    return big, view


def _check(hip, codec, w_old, region, new, seed=0):
    """One region of one stream, host stream and host source: the scrambled
    stream must come back with exactly the intersecting blocks replaced."""
    region = _norm(region, codec.shape)
    maxbits, off = codec.params[1], codec.bit_offset
    new = new[tuple(slice(lo, hi) for lo, hi in region)]
    w_img, cls = _expect(codec, w_old, region, new)
    rng = np.random.default_rng(seed)
    start = _scramble(w_old, cls, maxbits, off, rng)
    want = _splice(start, w_img, np.nonzero(cls)[0], maxbits, off)
    buf = np.concatenate([np.full(NSENT, SENT), start, np.full(NSENT, SENT)])
    stream = buf[NSENT:NSENT + len(start)]
    big, view = _strided_source(new)
    job = _job(codec.shape, TYPES[codec.dtype], codec.params, codec.coded)
    got = _call(hip, job, region, view.ctypes.data, [s // codec.dtype.itemsize for s in view.strides],
                stream.ctypes.data, len(start), off)
    assert (buf[:NSENT] == SENT).all() and (buf[-NSENT:] == SENT).all(), (region, "sentinel words written")
    bad = np.nonzero(_bits(stream) != _bits(want))[0]
    if bad.size:
        blocks = sorted({int((b - off) // maxbits) for b in bad})
        raise AssertionError((region, "stream differs in blocks", blocks[:10],
                              [int(cls[b]) if 0 <= b < len(cls) else None for b in blocks[:10]]))
    assert got == int((cls != 0).sum()) == _blocks(region, codec.coded, codec.shape), (region, "blocks_written")
    return want


def _rate_params(rate, dtype, dims):
    return params_rate(rate, TYPES[np.dtype(dtype)], dims)


# ---------------------------------------------------------------------------
# 1. 3D modes
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rate", [16, 8, 5, 3.25])
def test_regions_match_oracle_3d(hip, oracle, dtype, rate):
    rng = np.random.default_rng(zlib.crc32(repr((rate, np.dtype(dtype).name)).encode()))
    a = _special_field(SHAPE, dtype, rng)
    new = _special_field(SHAPE, dtype, rng)
    codec = _Codec(oracle, SHAPE, dtype, _rate_params(rate, dtype, 3))
    assert codec.params[1] == {16: 1024, 8: 512, 5: 320, 3.25: 208}[rate]
    w_old = codec.compress(a)
    for k, region in enumerate(REGIONS):
        _check(hip, codec, w_old, region, new, seed=k)


# 2. rows crossing waves and workgroups
@pytest.mark.parametrize("dtype,params", [(np.float32, params_rate(12, TYPE_FLOAT, 3)),
                                          (np.float64, (768, 768, 32, ZFP_MIN_EXP))])
def test_long_rows_cross_waves_and_workgroups(hip, oracle, dtype, params):
    """75 blocks per x-row; f64 with maxprec 32 is the planes-32..63 coder."""
    shape = (8, 8, 300)
    rng = np.random.default_rng(5)
    a = _special_field(shape, dtype, rng)
    new = _special_field(shape, dtype, rng)
    codec = _Codec(oracle, shape, dtype, params)
    w_old = codec.compress(a)
    for k, region in enumerate([((0, 8), (0, 8), (2, 299)), ((1, 6), (2, 7), (250, 300))]):
        _check(hip, codec, w_old, region, new, seed=k)


# 3. header offset
def test_stream_behind_a_header(hip, oracle):
    """Blocks start at bit 96: the 96 bits below stay, every block straddles words."""
    shape = (20, 24, 36)
    rng = np.random.default_rng(11)
    a = rng.standard_normal(shape).astype(np.float32)
    new = rng.standard_normal(shape).astype(np.float32)
    codec = _Codec(oracle, shape, np.float32, params_rate(8, 0, 3), bit_offset=96)
    w_old = codec.compress(a)
    for k, region in enumerate([((1, 18), (3, 23), (5, 34)), ((7, 8), None, (2, 35)), (None, None, None)]):
        _check(hip, codec, w_old, region, new, seed=k)


# 4. coded chunk inside a larger field
def test_coded_chunk_inside_a_larger_field(hip, oracle):
    shape = (24, 24, 48)
    coded = [(8, 20), (4, 24), (12, 40)]
    rng = np.random.default_rng(3)
    a = _special_field(shape, np.float32, rng)
    new = _special_field(shape, np.float32, rng)
    codec = _Codec(oracle, shape, np.float32, params_rate(8, TYPE_FLOAT, 3), coded=coded)
    w_old = codec.compress(a)
    for k, region in enumerate([((8, 13), (4, 11), (12, 30)),     # low corner at the box's f
                                ((10, 19), (9, 22), (17, 39)),    # interior
                                ((8, 20), (4, 24), (12, 40))]):   # the whole box
        _check(hip, codec, w_old, region, new, seed=k)


# 5. 1D / 2D
@pytest.mark.parametrize("rate", [8, 3.25])
@pytest.mark.parametrize("dtype,shape,region", [(np.float32, (13, 37), ((2, 11), (5, 34))),
                                                (np.float64, (70,), ((3, 66),))])
def test_1d_2d_floats_match_oracle(hip, oracle, dtype, shape, region, rate):
    """1D maxbits 32 and 13: several blocks share one word, every write is a merge."""
    rng = np.random.default_rng(29)
    a = (rng.standard_normal(shape) * 100).astype(dtype)
    new = (rng.standard_normal(shape) * 100).astype(dtype)
    codec = _Codec(oracle, shape, dtype, _rate_params(rate, dtype, len(shape)))
    w_old = codec.compress(a)
    one = tuple((n // 2, n // 2 + 1) for n in shape)
    for k, r in enumerate((region, (None,) * len(shape), one)):
        _check(hip, codec, w_old, r, new, seed=k)


@pytest.mark.parametrize("dtype,shape,region", [(np.int32, (70,), ((3, 66),)),
                                                (np.int64, (13, 37), ((2, 11), (5, 34)))])
def test_1d_2d_integers_match_reference(hip, ref_capi, dtype, shape, region):
    a = _int_field(shape, dtype, 31)
    new = _int_field(shape, dtype, 37)
    codec = _RefCodec(ref_capi, shape, dtype, 8)
    w_old = codec.compress(a)
    for k, r in enumerate((region, (None,) * len(shape))):
        _check(hip, codec, w_old, r, new, seed=k)


# 6. memory kinds
@pytest.mark.parametrize("region", [((3, 19), (5, 22), (6, 70)),   # scalar loads, a read-modify-write shell
                                    ((4, 21), (0, 26), (8, 72))])  # block-aligned low x: 16-byte rows of a device source
def test_host_and_device_memory(hip, oracle, region):
    """The four combinations of host or device stream and source agree (the
    source a strided view inside a larger array)."""
    import torch
    rng = np.random.default_rng(23)
    a = _special_field(SHAPE, np.float32, rng)
    new = _special_field(SHAPE, np.float32, rng)
    codec = _Codec(oracle, SHAPE, np.float32, params_rate(3.25, TYPE_FLOAT, 3))
    maxbits = codec.params[1]
    w_old = codec.compress(a)
    region = _norm(region, SHAPE)
    part = new[tuple(slice(lo, hi) for lo, hi in region)]
    w_img, cls = _expect(codec, w_old, region, part)
    start = _scramble(w_old, cls, maxbits, 0, rng)
    want = _splice(start, w_img, np.nonzero(cls)[0], maxbits, 0)
    job = _job(SHAPE, TYPE_FLOAT, codec.params)
    big, view = _strided_source(part)
    strides = [s // 4 for s in view.strides]
    d_big = torch.from_numpy(big).cuda()
    for dev_stream in (False, True):
        for dev_src in (False, True):
            buf = np.concatenate([np.full(NSENT, SENT), start, np.full(NSENT, SENT)])
            d_buf = torch.from_numpy(buf.view(np.int64)).cuda() if dev_stream else None
            wptr = d_buf.data_ptr() + 8 * NSENT if dev_stream else buf[NSENT:].ctypes.data
            sptr = d_big.data_ptr() + (view.ctypes.data - big.ctypes.data) if dev_src else view.ctypes.data
            got = _call(hip, job, region, sptr, strides, wptr, len(start), 0)
            if dev_stream:
                torch.cuda.synchronize()
                buf = d_buf.cpu().numpy().view(np.uint64)
            assert (buf[:NSENT] == SENT).all() and (buf[-NSENT:] == SENT).all(), (dev_stream, dev_src)
            assert buf[NSENT:-NSENT].tobytes() == want.tobytes(), (dev_stream, dev_src)
            assert got == int((cls != 0).sum())


def test_host_source_with_x_stride_and_negative_y_stride(hip, oracle):
    """A host source whose rows are not contiguous or run backwards gives the
    stream of a contiguous copy of the same values, word for word."""
    shape = (9, 10, 13)  # partial blocks on every axis
    region = [(2, 7), (1, 9), (3, 12)]
    rng = np.random.default_rng(61)
    a = _special_field(shape, np.float32, rng)
    new = np.ascontiguousarray(_special_field(shape, np.float32, rng)[tuple(slice(lo, hi) for lo, hi in region)])
    codec = _Codec(oracle, shape, np.float32, params_rate(8, TYPE_FLOAT, 3))
    w_old = codec.compress(a)
    job = _job(shape, TYPE_FLOAT, codec.params)

    def encode(src):
        w = w_old.copy()
        got = _call(hip, job, region, src.ctypes.data, [s // 4 for s in src.strides], w.ctypes.data, len(w), 0)
        assert got == _blocks(region, None, shape)
        return w

    want = encode(new)
    assert want.tobytes() != w_old.tobytes()
    for name, _, view in _strided_views(list(new.shape), np.float32):
        view[...] = new
        assert encode(view).tobytes() == want.tobytes(), name


# 7. chained updates
def test_chained_updates_on_a_device_stream(hip, oracle):
    import torch
    rng = np.random.default_rng(53)
    shape = SHAPE
    a = _special_field(shape, np.float32, rng)
    codec = _Codec(oracle, shape, np.float32, params_rate(8, TYPE_FLOAT, 3))
    maxbits = codec.params[1]
    want = codec.compress(a)
    d_words = torch.from_numpy(want.view(np.int64).copy()).cuda()
    job = _job(shape, TYPE_FLOAT, codec.params)
    for region in (((2, 14), (3, 17), (10, 50)), ((9, 21), (0, 26), (37, 66))):
        new = _special_field(shape, np.float32, rng)[tuple(slice(lo, hi) for lo, hi in region)]
        w_img, cls = _expect(codec, want, list(region), new)
        want = _splice(want, w_img, np.nonzero(cls)[0], maxbits, 0)
        src = np.ascontiguousarray(new)
        _call(hip, job, list(region), src.ctypes.data, [s // 4 for s in src.strides], d_words.data_ptr(), len(want), 0)
    torch.cuda.synchronize()
    assert d_words.cpu().numpy().view(np.uint64).tobytes() == want.tobytes()
    out = np.zeros(shape, dtype=np.float32)
    job.s[0], job.s[1], job.s[2] = 1, shape[2], shape[2] * shape[1]
    end = ctypes.c_uint64(0)
    assert hip.zfp_hip_decompress(ctypes.byref(job), out.ctypes.data, d_words.data_ptr(), len(want), 0, -1, None,
                                  ctypes.byref(end)) == 1, hip.zfp_hip_last_error().decode()
    assert out.tobytes() == codec.decompress(want).tobytes()


# ---------------------------------------------------------------------------
# 8. zfpy
def test_zfpy_compress_region(oracle):
    import zfpy
    rng = np.random.default_rng(41)
    a = rng.standard_normal(SHAPE).astype(np.float32)
    new = rng.standard_normal((16, 17, 64)).astype(np.float32)
    region = (slice(3, 19), slice(5, 22), slice(6, 70))
    box = [(3, 19), (5, 22), (6, 70)]
    s0 = zfpy.compress_numpy(a, rate=8)
    hbits = 96
    params = params_rate(8, 0, 3)
    codec = _Codec(oracle, SHAPE, np.float32, params, bit_offset=hbits)
    w_old = np.frombuffer(s0, dtype=np.uint64).copy()
    # (the oracle's stream has zeros where the header is: block bits only)
    assert _bits(codec.compress(a))[hbits:].tobytes() == _bits(w_old)[hbits:].tobytes()
    w_img, cls = _expect(codec, w_old, box, new)
    want = _splice(w_old, w_img, np.nonzero(cls)[0], params[1], hbits)
    s = bytearray(s0)
    view = np.empty((16, 17, 70), dtype=np.float32)[:, :, 3:67]  # strided values
    view[...] = new
    assert zfpy.compress_region(s, region, view) == int((cls != 0).sum())
    assert bytes(s) == want.tobytes()
    assert zfpy.decompress_region(s, region).tobytes() == \
        np.ascontiguousarray(codec.decompress(want)[region]).tobytes()
    # a writable memoryview and a uint8 ndarray are updated in place as well
    for make in (lambda b: memoryview(bytearray(b)), lambda b: np.frombuffer(bytearray(b), dtype=np.uint8)):
        t = make(s0)
        zfpy.compress_region(t, region, new)
        assert bytes(t) == want.tobytes()
    with pytest.raises(TypeError):
        zfpy.compress_region(bytes(s0), region, new)
    with pytest.raises(TypeError):
        zfpy.compress_region(memoryview(bytes(s0)), region, new)
    with pytest.raises(ValueError):
        zfpy.compress_region(bytearray(zfpy.compress_numpy(a, precision=16)), region, new)
    before = bytes(s)
    with pytest.raises(TypeError):
        zfpy.compress_region(s, region, new.astype(np.float64))
    with pytest.raises(ValueError):
        zfpy.compress_region(s, region, new[:, :, :60])
    assert bytes(s) == before


# 9. zfp_parallel
def test_zfp_parallel_compress_region(oracle):
    import zfpy
    shape = (64, 64, 96)
    rng = np.random.default_rng(43)
    idx = np.indices(shape, dtype=np.float32)
    a = (np.sin(0.05 * idx[0]) + np.cos(0.07 * idx[1]) * np.sin(0.03 * idx[2])
         + 1e-3 * rng.standard_normal(shape)).astype(np.float32)
    zp = zfpy.zfp_parallel(shape, "float32", nparts=8)
    zp.get_numpy_array()[...] = a
    streams = list(zp.compress(nthreads=8, rate=8))
    boxes = zp.get_chunkit().boxes
    assert len(boxes) == 8
    params = params_rate(8, 0, 3)
    hbits = 96
    coded = [list(reversed(b[:3])) for b in boxes]  # numpy axis order
    codecs = [_Codec(oracle, shape, np.float32, params, coded=[tuple(c) for c in cd], bit_offset=hbits)
              for cd in coded]
    want = [np.frombuffer(s, dtype=np.uint64).copy() for s in streams]
    straddle = (slice(5, 61), slice(3, 62), slice(7, 90))
    x, y, z = boxes[3][:3]  # one chunk's box (x first)
    inside = (slice(z[0] + 1, z[1] - 1), slice(y[0] + 2, y[1] - 1), slice(x[0] + 3, x[1] - 2))

    def expect(region, new):
        """the oracle-built chunk streams after region <- new; the chunks it touches"""
        box = [(s.start, s.stop) for s in region]
        hit = []
        for i, cd in enumerate(coded):
            part = [(max(f, cf), min(e, ce)) for (f, e), (cf, ce) in zip(box, cd)]
            if not all(f < e for f, e in part):
                continue
            hit.append(i)
            sub = new[tuple(slice(f - f0, e - f0) for (f, e), (f0, _) in zip(part, box))]
            w_img, cls = _expect(codecs[i], want[i], part, sub)
            want[i] = _splice(want[i], w_img, np.nonzero(cls)[0], params[1], hbits)
        return hit

    # the region straddles all eight chunks; values given
    new1 = rng.standard_normal((56, 59, 83)).astype(np.float32)
    assert expect(straddle, new1) == list(range(8))
    out = zp.compress_region(straddle, new1, nthreads=8)
    assert out is zp._compress_data
    for i in range(8):
        assert isinstance(out[i], bytes) and out[i] == want[i].tobytes(), i
    # one strictly inside chunk 3; values from the shared array
    before = list(zp._compress_data)
    new2 = rng.standard_normal(shape).astype(np.float32)
    zp.get_numpy_array()[...] = new2
    assert expect(inside, np.ascontiguousarray(new2[inside])) == [3]
    zp.compress_region(inside, nthreads=8)
    for i in range(8):
        assert zp._compress_data[i] == want[i].tobytes(), i
        assert (zp._compress_data[i] is before[i]) == (i != 3), i
    zp.decompress(nthreads=8)
    full = np.zeros(shape, dtype=np.float32)
    for i, cd in enumerate(coded):
        sl = tuple(slice(f, e) for f, e in cd)
        full[sl] = codecs[i].decompress(want[i])[sl]
    assert np.array(zp.get_numpy_array()).tobytes() == full.tobytes()
    # variable rate, and no compressed data
    zp.compress(nthreads=8, precision=16)
    with pytest.raises(RuntimeError):
        zp.compress_region(inside)
    zp2 = zfpy.zfp_parallel(shape, "float32", nparts=8)
    with pytest.raises(RuntimeError):
        zp2.compress_region(inside)
