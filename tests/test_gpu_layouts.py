"""Field layout matrix: strides, offsets and chunk boxes of 1D-4D fields on the GPU.

Every kernel and the host shim take a field as extents, signed element strides,
a chunk box and a base pointer; the geometry code (plan_job, copy_box,
block_pos, the gathers and scatters) is shared by all codecs.  These tests run
the layouts of tests/layouts.py through every path that takes one:

  host field      zfp_compress / zfp_decompress with the field's own strides
  chunk boxes     zfp_compress_chunk / zfp_decompress_chunk, aligned or not
  device field    a raw device pointer plus strides, device stream
  slab pipeline   a sub-box of a host field through the slab pipeline

float32 / float64 are checked against the oracle (pinned to the reference for
every layout in test_oracle.py), int32 / int64 against the reference library
called with the same strided view.  A decode goes into a view of a buffer
pre-filled with a sentinel bit pattern: the view must hold the reference's
values bit for bit and every other element of the buffer must still hold the
sentinel.
"""
import ctypes
import zlib

import numpy as np
import pytest

import layouts
from layouts import FIXED_RATE, SHAPES, bits, guard_intact, make_view, zfp_strides
from pyoracle import TYPE_DOUBLE, TYPE_FLOAT, params_precision, params_rate, params_reversible
from test_gpu_pipeline import _field as smooth_field, _pipelined, slabs  # noqa: F401  (slabs: env fixture)
from test_gpu_types import _field as int_field

pytestmark = pytest.mark.gpu

TYPES = {np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.float32): 3, np.dtype(np.float64): 4}
DTYPES = ["float32", "float64", "int32", "int64"]

# Host-resident decode copies the decoded box back row by row and needs unit x
# stride for that (copy_box); these layouts it refuses, every other one works.
# (In 1D the outermost axis is x, so rev_outer is a negative x stride there.)
HOST_DECODE_REFUSED = {(1, "interleaved"), (1, "rev_x"), (1, "rev_outer"), (1, "rev_all"),
                       (2, "interleaved"), (2, "transposed"), (2, "rev_x"), (2, "rev_all"),
                       (3, "interleaved"), (3, "transposed"), (3, "rev_x"), (3, "rev_all"),
                       (4, "interleaved"), (4, "transposed"), (4, "rev_x"), (4, "rev_all")}
HOST_DECODE_WORKS = {(d, l) for d in (1, 2, 3, 4) for l in layouts.layouts_for(d)} - HOST_DECODE_REFUSED
assert {(d, l) for d in (2, 3, 4) for l in ("dense", "pad4", "pad3", "shift1", "rev_y", "rev_outer")} | \
       {(1, l) for l in ("dense", "pad4", "pad3", "shift1")} == HOST_DECODE_WORKS


def _modes(dims, layout):
    m = [("rate", FIXED_RATE[dims]), ("precision", 18)]
    if layout in ("dense", "pad3", "rev_all"):
        m.append(("reversible", None))
    return m


def _params(mode, param, ztype, dims):
    if mode == "rate":
        return params_rate(param, ztype, dims)
    return params_precision(param) if mode == "precision" else params_reversible()


_DATA = {}


def _data(dims, dtype):
    """The dense field of one (dims, dtype): computed once, never changed."""
    key = (dims, np.dtype(dtype).name)
    if key not in _DATA:
        dtype = np.dtype(dtype)
        seed = zlib.crc32(repr(key).encode())
        if dtype.kind == "f":
            a = layouts.special_field(SHAPES[dims], dtype, np.random.default_rng(seed))
        else:
            a = int_field(SHAPES[dims], dtype, seed)
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


class _Reference:
    """The oracle for floats, the reference library for integers, behind one face."""

    def __init__(self, request, dtype):
        self.isf = np.dtype(dtype).kind == "f"
        self.lib = request.getfixturevalue("oracle" if self.isf else "ref_capi")

    def encode(self, view, mode, param, box=None):
        if not self.isf:
            return self.lib.compress(view, mode, param, chunk=box, strided=True)
        params = _params(mode, param, TYPES[view.dtype], view.ndim)
        b4 = None if box is None else list(box) + [(0, 0)] * (4 - view.ndim)
        words, end = self.lib.compress_words(view, params, box=b4, strides=zfp_strides(view), base=view.ctypes.data)
        return words.view(np.uint8)[: (end + 63) // 64 * 8].tobytes()

    def decode_into(self, data, buf, view, mode, param, box=None):
        """Decode `data` (the chunk `box` of it) through `view` into `buf`."""
        if not self.isf:
            _, n = self.lib.decompress(data, view.shape, view.dtype, mode, param, out=view, strided=True, chunk=box)
            assert n == len(data)
            return
        params = _params(mode, param, TYPES[view.dtype], view.ndim)
        b4 = None if box is None else list(box) + [(0, 0)] * (4 - view.ndim)
        self.lib.decompress_words(np.frombuffer(data, dtype=np.uint64), view.shape, view.dtype, params, box=b4,
                                  out=buf, strides=zfp_strides(view), base=view.ctypes.data)


def _free_index(product, *indexes):
    for idx in set(indexes) | {product.last_index}:
        if idx:
            product.lib.zfp_hip_index_free(idx)
    product.last_index = None


# ---------------------------------------------------------------------------
# a, b: host field, every layout
HOST_CASES = [(d, l, t) for d in (1, 2, 3, 4) for l in layouts.layouts_for(d) for t in DTYPES]


@pytest.mark.parametrize("dims,layout,dtype", HOST_CASES)
def test_host_field_layouts(product, request, dims, layout, dtype):
    """Encode of a strided host field equals the reference bytes; decode of the
    reference stream into a strided host view, with the encoder's index and
    with a scan, equals the reference decode and writes nothing outside the
    view -- or, for the layouts listed in HOST_DECODE_REFUSED, is refused before
    the destination is touched, leaving the thread fit for the next call."""
    a = _data(dims, dtype)
    ref = _Reference(request, dtype)
    refused = (dims, layout) in HOST_DECODE_REFUSED
    assert refused != ((dims, layout) in HOST_DECODE_WORKS)
    for mode, param in _modes(dims, layout):
        buf, view = make_view(a, layout)
        held = bits(buf).tobytes()
        want = ref.encode(view, mode, param)
        product.last_index = None
        got = product.compress(view, mode, param, strided=True)
        index = product.last_index
        try:
            assert got == want, (mode, "encode")
            assert bits(buf).tobytes() == held, (mode, "encode changed the field")
            rbuf, rview = make_view(a, layout, fill=False)
            ref.decode_into(want, rbuf, rview, mode, param)
            for idx in ((index, None) if index else (None,)):
                dbuf, dview = make_view(a, layout, fill=False)
                before = bits(dbuf).tobytes()
                _, n = product.decompress(want, a.shape, a.dtype, mode, param, out=dview, strided=True, index=idx)
                if refused:
                    assert n == 0, (mode, "a refused layout decoded")
                    assert b"stride" in product.lib.zfp_hip_last_error(), mode
                    assert bits(dbuf).tobytes() == before, (mode, "a refused decode wrote to the destination")
                    out, n = product.decompress(want, a.shape, a.dtype, mode, param, index=idx)
                    assert n == len(want), (mode, "dense decode after a refusal")
                    assert bits(out).tobytes() == bits(np.ascontiguousarray(rview)).tobytes(), mode
                else:
                    assert n == len(want), (mode, idx is None, product.lib.zfp_hip_last_error())
                    assert bits(dview).tobytes() == bits(rview).tobytes(), (mode, idx is None, "decode")
                    assert guard_intact(dbuf, dview), (mode, idx is None, "decode wrote outside the view")
        finally:
            _free_index(product, index)


# ---------------------------------------------------------------------------
# c: chunk boxes through zfp_compress_chunk / zfp_decompress_chunk
CHUNK_CASES = [(d, l, t, b) for d in (1, 2, 3, 4) for l in ("dense", "pad3") for t in DTYPES
               for b in layouts.CHUNK_BOXES[d]]


@pytest.mark.parametrize("dims,layout,dtype,boxname", CHUNK_CASES)
def test_chunk_boxes_through_c_api(product, request, dims, layout, dtype, boxname):
    """A chunk encode equals the reference's encode of the same box; a chunk
    decode writes exactly what the reference's chunk decode writes -- the
    chunk's whole blocks clipped by the field, not by the chunk's end -- and
    the rest of the buffer keeps the sentinel.  Origins off a multiple of 4
    included (oracle and reference agree on them: checked on the CPU)."""
    a = _data(dims, dtype)
    box = layouts.CHUNK_BOXES[dims][boxname]
    ref = _Reference(request, dtype)
    written = layouts.chunk_written(a.shape, box)
    for mode, param in (("rate", FIXED_RATE[dims]), ("precision", 18)):
        buf, view = make_view(a, layout)
        want = ref.encode(view, mode, param, box)
        product.last_index = None
        got = product.compress(view, mode, param, chunk=box, strided=True)
        index = product.last_index
        try:
            assert got == want, (mode, "encode")
            rbuf, rview = make_view(a, layout, fill=False)
            ref.decode_into(want, rbuf, rview, mode, param, box)
            assert guard_intact(rbuf, rview, written)  # the reference itself writes whole clipped blocks
            for idx in ((index, None) if index else (None,)):
                dbuf, dview = make_view(a, layout, fill=False)
                _, n = product.decompress(want, a.shape, a.dtype, mode, param, out=dview, strided=True, chunk=box,
                                          index=idx)
                assert n == len(want), (mode, idx is None, product.lib.zfp_hip_last_error())
                assert bits(dview)[written].tobytes() == bits(rview)[written].tobytes(), (mode, idx is None)
                assert guard_intact(dbuf, dview, written), (mode, idx is None, "decode wrote outside the chunk's blocks")
                assert bits(dbuf).tobytes() == bits(rbuf).tobytes(), (mode, idx is None)
        finally:
            _free_index(product, index)


# ---------------------------------------------------------------------------
# d: device-resident field and stream
def _device_field(lib, ptr, dtype, shape, strides):
    n = list(reversed(shape))
    make = {2: lib.zfp_field_2d, 3: lib.zfp_field_3d, 4: lib.zfp_field_4d}[len(n)]
    field = make(ctypes.c_void_p(ptr), TYPES[np.dtype(dtype)], *n)
    {2: lib.zfp_field_set_stride_2d, 3: lib.zfp_field_set_stride_3d, 4: lib.zfp_field_set_stride_4d}[len(n)](
        field, *strides[: len(n)])
    return field


DEVICE_CASES = [(d, t, l) for d, t in ((2, "float64"), (3, "float32"), (4, "float32")) for l in layouts.layouts_for(d)]


@pytest.mark.parametrize("dims,dtype,layout", DEVICE_CASES)
def test_device_field_layouts(product, oracle, dims, dtype, layout):
    """A raw device pointer (the address of logical element 0) plus signed strides,
    stream on the device: the kernels take every layout, the ones the host path
    refuses included, and encode and decode bit-exactly with the guard intact."""
    torch = pytest.importorskip("torch")
    a = _data(dims, dtype)
    lib = product.lib
    for mode, param in _modes(dims, layout):
        params = _params(mode, param, TYPES[a.dtype], dims)
        buf, view = make_view(a, layout)
        st = zfp_strides(view)
        words, end = oracle.compress_words(view, params, strides=st, base=view.ctypes.data)
        want = words.view(np.uint8)[: (end + 63) // 64 * 8].tobytes()
        rbuf, rview = make_view(a, layout, fill=False)
        oracle.decompress_words(words, a.shape, a.dtype, params, out=rbuf, strides=st, base=rview.ctypes.data)
        d_src = torch.from_numpy(bits(buf).view(np.uint8).copy()).cuda()
        d_dst = torch.from_numpy(bits(rbuf).view(np.uint8).copy()).cuda()
        d_dst[:] = layouts.SENTINEL_BYTE
        off = view.ctypes.data - buf.ctypes.data  # bytes from the buffer's start to logical element 0
        field = _device_field(lib, d_src.data_ptr() + off, a.dtype, a.shape, st)
        zs = lib.zfp_stream_open(None)
        product.set_mode(zs, mode, param, TYPES[a.dtype], dims)
        cap = lib.zfp_stream_maximum_size(zs, field) + 64
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        bs = lib.stream_open(ctypes.c_void_p(d_out.data_ptr()), cap)
        lib.zfp_stream_set_bit_stream(zs, bs)
        try:
            n = lib.zfp_compress(zs, field)
            assert n == len(want), (mode, product.lib.zfp_hip_last_error())
            assert d_out[:n].cpu().numpy().tobytes() == want, (mode, "encode")
            assert d_src.cpu().numpy().tobytes() == bits(buf).tobytes(), (mode, "encode changed the field")
            lib.zfp_field_set_pointer(field, ctypes.c_void_p(d_dst.data_ptr() + off))
            lib.stream_rewind(bs)
            assert lib.zfp_decompress(zs, field) == n, (mode, product.lib.zfp_hip_last_error())
            back = d_dst.cpu().numpy().view(buf.dtype)
            dview = np.lib.stride_tricks.as_strided(back[off // back.itemsize:], shape=view.shape, strides=view.strides)
            assert bits(dview).tobytes() == bits(rview).tobytes(), (mode, "decode")
            assert guard_intact(back, dview), (mode, "decode wrote outside the view")
        finally:
            lib.stream_close(bs)
            lib.zfp_stream_close(zs)
            lib.zfp_field_free(field)


# ---------------------------------------------------------------------------
# e: a sub-box through the slab pipeline
@pytest.mark.parametrize("mode,param", [("rate", 12), ("precision", 16)])
def test_pipelined_sub_box(product, oracle, slabs, mode, param):
    """A chunk restricted in x and y (block-aligned origin, ends inside the
    field) of a host field large enough for the slab pipeline.  make_slabs cuts
    any box of a densely stored field along its outermost axis and keeps the
    box's x and y range in every slab, so the pipeline runs (asserted) for the
    encode, and for the decode whenever the slab boundaries are known up front
    (fixed rate, or the encoder's index); a decode that has to scan the stream
    takes the one-shot path.  Each slab's download is the row-by-row copy of
    its box."""
    a = smooth_field((72, 64, 128), np.float32, 17)
    box = [(4, 100), (8, 56), (0, 72)]  # 24 x 12 blocks a layer: even, so 14-layer slabs hold whole waves
    params = _params(mode, param, TYPE_FLOAT, 3)
    buf, view = make_view(a, "dense")
    written = layouts.chunk_written(a.shape, box)
    words, end = oracle.compress_words(view, params, box=box + [(0, 0)])
    want = words.view(np.uint8)[: (end + 63) // 64 * 8].tobytes()
    rbuf, rview = make_view(a, "dense", fill=False)
    oracle.decompress_words(words, a.shape, a.dtype, params, box=box + [(0, 0)], out=rbuf, base=rview.ctypes.data)
    product.last_index = None
    got = product.compress(view, mode, param, chunk=box, strided=True)
    index = product.last_index
    try:
        assert _pipelined(product), "the slab pipeline did not run (encode)"
        assert got == want
        for idx in ((index, None) if index else (None,)):
            dbuf, dview = make_view(a, "dense", fill=False)
            _, n = product.decompress(want, a.shape, a.dtype, mode, param, out=dview, strided=True, chunk=box, index=idx)
            assert n == len(want), product.lib.zfp_hip_last_error()
            assert _pipelined(product) == (mode == "rate" or idx is not None)
            assert bits(dbuf).tobytes() == bits(rbuf).tobytes(), (idx is None, "decode")
            assert guard_intact(dbuf, dview, written), (idx is None, "decode wrote outside the chunk's blocks")
    finally:
        _free_index(product, index)
