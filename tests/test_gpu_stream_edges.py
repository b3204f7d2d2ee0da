"""Stream buffer edges of zfp_hip_compress / zfp_hip_decompress (libzfp_hip.so at its C ABI).

The contract is the reference's (streams.py): an encode writes the bits from
bit_offset through the zero-padded last word and nothing else; the bits below
bit_offset in the start word are the caller's pending bits (head_word), not what
memory holds.  Every stream buffer here is prefilled with a position-dependent
non-zero pattern and carries four pattern words before word 0 and four beyond
the capacity; whole allocations are compared with streams.expected_image, so a
shared word ORed without being zeroed, a skipped word, a displaced copy and a
store one word past the stream (inside or outside the capacity) all show.

No case compares the product with itself: expected bits are the oracle's
(float, double), the reference library's (integer fields; those cases skip
without oracle/_ref) or the prefill.

Capacities are in words from the buffer start; `exact` is
(bit_offset + total + 63) // 64.  From zfp_hip_compress: with
worst_bits = bit_offset % 64 + nblocks * (maxbits for fixed rate, else the
mode's longest block), a device stream is written in place ("direct") iff
bit_offset // 64 + (worst_bits + 63) // 64 + 1 <= capacity_words, and is
otherwise coded into scratch and copied device to device ("staged"); a host
stream is always staged.

  fixed rate     worst_bits is the stream's own length: `exact` is staged,
                 `exact + 1`, `exact + 2` and `max + 8` are direct, and
                 `exact - 1` is refused before any GPU work
  variable rate  worst_bits is far above any stream of these fields: `exact`,
                 `exact + 1` and `exact + 2` are staged, `max + 8`
                 (zfp_stream_maximum_size in words, plus 8) is direct, and
                 `exact - 1` is refused after the encode, before the copy

so every device case list below has both sides of that condition.
"""
import ctypes
import zlib

import numpy as np
import pytest

import layouts
import streams
from pyoracle import params_rate
from streams import GUARD, Buffer, exact_words, head_bits_for
from test_gpu_region import LIB_HIP, TYPES, _job, _params

pytestmark = pytest.mark.gpu

OFFSETS = (0, 1, 63, 64, 100)
SHAPES = {1: [(37,), (1030,)], 2: [(13, 22), (45, 67)], 3: [(8, 12, 68), (18, 23, 130)],
          4: [(5, 6, 7, 9), (9, 6, 10, 13)]}
SLOTS3 = {"ZFP_HIP_SLOT_WORDS": "5"}                             # 3D: long blocks take the overflow pool
REDO3 = {"ZFP_HIP_SLOT_WORDS": "5", "ZFP_HIP_OVF_POOL": "7"}     # ... which runs out: the launch is redone
SLOTS4 = {"ZFP_HIP_SLOT_WORDS": "9"}                             # 4D: long blocks go through the patch kernel
REDO4 = {"ZFP_HIP_SLOT_WORDS": "9", "ZFP_HIP_OVF_POOL": "3"}     # 4D: the redo with full slots
PIPE = {"ZFP_HIP_PIPE_MIN_MB": "1", "ZFP_HIP_PIPE_SLAB_MB": "1"}


@pytest.fixture(scope="module")
def hip(product):
    lib = ctypes.CDLL(LIB_HIP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.zfp_hip_compress.restype = ctypes.c_int
    lib.zfp_hip_compress.argtypes = [vp, vp, vp, u64, u64, u64, ctypes.c_int, vp, vp]
    lib.zfp_hip_decompress.restype = ctypes.c_int
    lib.zfp_hip_decompress.argtypes = [vp, vp, vp, u64, u64, ctypes.c_int, vp, vp]
    lib.zfp_hip_index_create.restype = vp
    lib.zfp_hip_index_free.argtypes = [vp]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    lib.zfp_hip_last_scan.restype = ctypes.c_int
    lib.zfp_hip_last_scan.argtypes = [vp, vp]
    lib.zfp_hip_last_timing.restype = ctypes.c_int
    lib.zfp_hip_last_timing.argtypes = [vp, vp]
    return lib


# ---------------------------------------------------------------------------
# fields and references, computed once per (dtype, shape, mode, offset)
_FIELDS, _REFS, _DEVICE_FIELDS = {}, {}, {}


def _field(dtype, shape, rev=False):
    """Float fields with zero, NaN and denormal blocks and long blocks; integers
    at the edge of the range the mode takes."""
    dtype = np.dtype(dtype)
    key = (dtype.name, shape, rev and dtype.kind == "i")
    if key not in _FIELDS:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        if dtype.kind == "i":
            a = layouts.edge_ints(shape, dtype, rng, full_range=rev)
        else:
            a = layouts.special_field(shape, dtype, rng)
        a.setflags(write=False)
        _FIELDS[key] = a
    return _FIELDS[key]


def _device_field(a):
    import torch
    key = id(a)
    if key not in _DEVICE_FIELDS:
        _DEVICE_FIELDS[key] = torch.from_numpy(np.array(a)).cuda()
    return _DEVICE_FIELDS[key]


class Ref:
    """The reference stream of one field at one bit offset (words absolute, zeros
    below the offset), its end bit and its decode."""

    def __init__(self, words, end_bit, decoded):
        self.words, self.end_bit, self.decoded = words, end_bit, decoded
        self.exact = exact_words(end_bit)


def _ref(request, a, mode, param, bit_offset):
    key = (a.dtype.name, a.shape, mode, param, bit_offset, id(a))
    if key in _REFS:
        return _REFS[key]
    ztype = TYPES[a.dtype]
    params = _params(mode, param, ztype, a.ndim)
    if a.dtype.kind == "f":
        oracle = request.getfixturevalue("oracle")
        words, end = oracle.compress_words(a, params, bit_offset=bit_offset)
        dec, dend = oracle.decompress_words(words, a.shape, a.dtype, params, bit_offset=bit_offset)
        assert dend == end
    else:
        ref = request.getfixturevalue("ref_capi")
        data = ref.compress(np.array(a), mode, param, ztype=ztype, pad_bits=bit_offset)
        words = streams.as_words(data)
        dec, n = ref.decompress(data, a.shape, a.dtype, mode, param, ztype=ztype, pad_bits=bit_offset)
        assert n == len(data)
        if params[0] == params[1]:
            end = bit_offset + _nblocks(a.shape) * params[1]
        else:
            end = _ref_end_bit(ref, a, mode, param, bit_offset, len(words))
        assert exact_words(end) == len(words)
    r = Ref(words, end, dec)
    _REFS[key] = r
    return r


def _ref_end_bit(ref, a, mode, param, bit_offset, nwords):
    """The end bit of the reference library's variable-rate stream.  Its C API
    reports whole words only, so pad by k more bits until the stream takes one
    more word: then bit_offset + k + total == 64 * nwords + 1 (bisection, six
    compressions of a small field)."""
    lo, hi = 0, 64  # k = lo: still nwords words; k = hi: more
    while hi - lo > 1:
        k = (lo + hi) // 2
        n = len(ref.compress(np.array(a), mode, param, ztype=TYPES[a.dtype], pad_bits=bit_offset + k))
        lo, hi = (k, hi) if n == 8 * nwords else (lo, k)
    return 64 * nwords + 1 - hi


def _nblocks(shape):
    n = 1
    for v in shape:
        n *= (v + 3) // 4
    return n


def _dense_job(shape, ztype, params):
    j = _job(shape, ztype, params)
    s = 1
    for a in range(len(shape)):
        j.s[a] = s
        s *= j.n[a]
    return j


def _max_words(api, shape, ztype, mode, param):
    """zfp_stream_maximum_size for the field, in words."""
    lib = api.lib
    make = {1: lib.zfp_field_1d, 2: lib.zfp_field_2d, 3: lib.zfp_field_3d, 4: lib.zfp_field_4d}[len(shape)]
    field = make(None, ztype, *reversed(shape))
    zs = lib.zfp_stream_open(None)
    api.set_mode(zs, mode, param, ztype, len(shape))
    n = lib.zfp_stream_maximum_size(zs, field)
    lib.zfp_stream_close(zs)
    lib.zfp_field_free(field)
    assert n and n % 8 == 0
    return n // 8


def _compress(hip, job, field_ptr, buf, capacity, bit_offset, head, index=None):
    end = ctypes.c_uint64(0)
    rc = hip.zfp_hip_compress(ctypes.byref(job), field_ptr, buf.ptr, capacity, bit_offset, head, -1, index,
                              ctypes.byref(end))
    return rc, end.value


def _decompress(hip, job, a, dev_field, words_ptr, capacity, bit_offset, index):
    """Decode into a sentinel-filled host or device array; (rc, end_bit, bytes)."""
    out = np.empty(a.shape, dtype=a.dtype)
    out.view(np.uint8)[...] = 0xA5
    if dev_field:
        import torch
        d_out = torch.from_numpy(out).cuda()
        ptr = d_out.data_ptr()
    else:
        ptr = out.ctypes.data
    end = ctypes.c_uint64(0)
    rc = hip.zfp_hip_decompress(ctypes.byref(job), ptr, words_ptr, capacity, bit_offset, -1, index, ctypes.byref(end))
    if dev_field:
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
    return rc, end.value, out.tobytes()


def _scanned(hip):
    return hip.zfp_hip_last_scan(None, None) == 1


def _setenv(monkeypatch, env):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------
# encode matrix: (id, dtype, dims, mode, param, env)
def _case(dtype, dims, mode, param, env=None, tag=""):
    name = "%dd-%s-%s%s%s" % (dims, np.dtype(dtype).name, mode, "" if param is None else "-%g" % param, tag)
    return pytest.param(np.dtype(dtype).name, dims, mode, param, env, id=name)


ENCODE = []
ENCODE += [_case("f4", 3, "rate", r, tag="-aligned") for r in (1, 3, 8, 16, 32)]
ENCODE += [_case("f8", 3, "rate", r, tag="-aligned") for r in (16, 64)]
ENCODE += [_case(t, 3, "rate", r, tag="-general") for t in ("f4", "f8") for r in (3.25, 12.5)]
for env, tag in ((None, ""), (SLOTS3, "-overflow"), (REDO3, "-redo")):
    ENCODE += [_case("f4", 3, m, p, env, tag) for m, p in (("precision", 12), ("accuracy", 1e-3), ("reversible", None))]
    ENCODE += [_case("f8", 3, m, p, env, tag) for m, p in (("precision", 20), ("precision", 40), ("reversible", None))]
ENCODE += [_case("f4", 4, m, p) for m, p in (("rate", 8), ("rate", 3.25), ("precision", 20), ("reversible", None))]
ENCODE += [_case("f4", 4, "precision", 20, SLOTS4, "-patch"), _case("f4", 4, "reversible", None, SLOTS4, "-patch"),
           _case("f4", 4, "reversible", None, REDO4, "-redo")]
for t in ("f4", "f8", "i4", "i8"):
    prec = 14 if t[0] == "i" else 18
    ENCODE += [_case(t, d, m, p) for d in (1, 2)
               for m, p in (("rate", 8), ("rate", 12), ("precision", prec), ("reversible", None))]
ENCODE += [_case(t, d, m, p) for t in ("i4", "i8") for d in (3, 4) for m, p in (("rate", 8), ("reversible", None))]


def _placements(dtype, dims):
    """(device field, device stream, offsets, capacities): device with device and
    host with host over the whole matrix; the mixed ones on the 3D float cases."""
    # 3D f32/f64: offset 65 as well.  The aligned kernel with an unaligned start
    # pairs its 16-byte stores by the address of the start word (even: 1, 63;
    # odd: 65, 100) and shifts by whole dwords or not (1, 65 against 63, 100).
    offsets = OFFSETS + (65,) if dims == 3 and np.dtype(dtype).kind == "f" else OFFSETS
    full = (offsets, ("exact", "exact+1", "exact+2", "max+8"))
    out = [(True, True) + full, (False, False) + full]
    if dims == 3 and np.dtype(dtype) == np.float32:
        some = ((0, 63, 100), ("exact", "exact+1"))
        out += [(False, True) + some, (True, False) + some]
    return out


def _capacity(name, ref, max_words):
    return {"exact": ref.exact, "exact+1": ref.exact + 1, "exact+2": ref.exact + 2, "max+8": max_words + 8}[name]


@pytest.mark.parametrize("dtype,dims,mode,param,env", ENCODE)
def test_encode_writes_the_stream_and_nothing_else(hip, product, request, monkeypatch, dtype, dims, mode, param, env):
    """Return value 1, *end_bit the reference's, the whole allocation equal to
    expected_image; for variable rate the index the call filled decodes the
    stream (without a scan) to the reference's values."""
    _setenv(monkeypatch, env)
    dtype = np.dtype(dtype)
    ztype = TYPES[dtype]
    params = _params(mode, param, ztype, dims)
    fixed = params[0] == params[1]
    rng = np.random.default_rng(zlib.crc32(repr((dtype.name, dims, mode, param)).encode()))
    index = None if fixed else hip.zfp_hip_index_create()
    try:
        for shape in SHAPES[dims]:
            a = _field(dtype, shape, mode == "reversible")
            job = _dense_job(shape, ztype, params)
            max_words = _max_words(product, shape, ztype, mode, param)
            for dev_field, dev_stream, offsets, capacities in _placements(dtype, dims):
                fptr = _device_field(a).data_ptr() if dev_field else a.ctypes.data
                for off in offsets:
                    ref = _ref(request, a, mode, param, off)
                    for cname in capacities:
                        cap = _capacity(cname, ref, max_words)
                        what = (shape, "device" if dev_field else "host", "device" if dev_stream else "host", off, cname)
                        head = head_bits_for(rng, off)
                        buf = Buffer(cap, dev_stream)
                        rc, end = _compress(hip, job, fptr, buf, cap, off, head, index)
                        assert rc == 1, (what, hip.zfp_hip_last_error().decode())
                        assert end == ref.end_bit, what
                        buf.check(off, head, ref.words, end, what)
                        if not fixed:
                            rc, dend, got = _decompress(hip, job, a, dev_field, buf.ptr, cap, off, index)
                            assert rc == 1, (what, hip.zfp_hip_last_error().decode())
                            assert not _scanned(hip), (what, "the encoder's index was not used")
                            assert dend == end and got == ref.decoded.tobytes(), (what, "decode with the encoder's index")
    finally:
        if index:
            hip.zfp_hip_index_free(index)


# ---------------------------------------------------------------------------
# the slab pipeline: the word shared by two slabs, nothing to spare after the last
PIPE_SHAPE = (64, 64, 80)


def _pipelined(hip):
    """The last call took the slab pipeline (it reports wall time only)."""
    k, t = ctypes.c_double(-1), ctypes.c_double(-1)
    return hip.zfp_hip_last_timing(ctypes.byref(k), ctypes.byref(t)) == 1 and k.value == 0.0


@pytest.mark.parametrize("mode,param", [("rate", 3.25), ("precision", 18)])
def test_slab_pipeline_at_exact_capacity(hip, request, monkeypatch, mode, param):
    """Host field, host stream, bit offset 100, capacity `exact`, slabs of 1 MB
    (two slabs, 3840 and 1280 blocks; at rate 3.25 the first ends at bit 36 of
    a word): Head::keep merges the word two slabs share.  The slabs are coded
    into scratch that the context keeps, so another field goes through first
    and leaves it dirty.  Then capacity `exact - 1`: fixed
    rate is refused before any work (buffer untouched), variable rate after
    earlier slabs may have been downloaded (nothing at or past the capacity and
    nothing before the stream changes); the same thread then compresses again."""
    _setenv(monkeypatch, PIPE)
    a = _field(np.float32, PIPE_SHAPE)
    params = _params(mode, param, 3, 3)
    fixed = params[0] == params[1]
    job = _dense_job(PIPE_SHAPE, 3, params)
    off = 100
    ref = _ref(request, a, mode, param, off)
    rng = np.random.default_rng(77)
    index = None if fixed else hip.zfp_hip_index_create()
    try:
        # the slabs are coded into device scratch that the context keeps between
        # calls: another field's stream first, so that it is not zero either
        other = np.ascontiguousarray(a[::-1, ::-1, ::-1])
        buf = Buffer(2 * ref.exact, False)
        rc, _ = _compress(hip, job, other.ctypes.data, buf, 2 * ref.exact, 37, 0)
        assert rc == 1 and _pipelined(hip), hip.zfp_hip_last_error().decode()
        for cap in (ref.exact, ref.exact - 1, ref.exact):
            head = head_bits_for(rng, off)
            buf = Buffer(cap, False)
            rc, end = _compress(hip, job, a.ctypes.data, buf, cap, off, head, index)
            if cap < ref.exact:
                assert rc == 0 and hip.zfp_hip_last_error(), cap
                _check_refused(buf, off, strict=fixed)
                continue
            assert rc == 1, hip.zfp_hip_last_error().decode()
            assert _pipelined(hip), "the call did not take the slab pipeline"
            assert end == ref.end_bit
            buf.check(off, head, ref.words, end, (mode, param, cap))
            if not fixed:
                rc, dend, got = _decompress(hip, job, a, False, buf.ptr, cap, off, index)
                assert rc == 1, hip.zfp_hip_last_error().decode()
                assert _pipelined(hip) and not _scanned(hip)
                assert dend == end and got == ref.decoded.tobytes()
    finally:
        if index:
            hip.zfp_hip_index_free(index)


# ---------------------------------------------------------------------------
# capacity refusals
def _check_refused(buf, bit_offset, strict):
    """After a refused call.  strict: the whole allocation is the prefill.
    Otherwise every word at or past the capacity and every word before the
    stream's start word is; words inside the capacity are unspecified."""
    got = buf.read()
    want = buf.prefill
    if not strict:
        got, want = got.copy(), want.copy()
        lo, hi = GUARD + bit_offset // 64, GUARD + buf.capacity
        got[lo:hi] = 0
        want[lo:hi] = 0
    msg = streams.difference(got, want, bit_offset, bit_offset, buf.capacity)
    assert msg is None, ("refused call wrote", msg)


REFUSALS = [_case("f4", 3, "rate", 8, tag="-aligned"), _case("f4", 3, "rate", 3.25, tag="-general"),
            _case("f4", 4, "rate", 3.25), _case("f8", 1, "rate", 12),
            _case("f4", 3, "precision", 12), _case("f4", 4, "reversible", None)]


@pytest.mark.parametrize("dtype,dims,mode,param,env", REFUSALS)
def test_capacity_one_word_short_is_refused(hip, request, dtype, dims, mode, param, env):
    """Capacity `exact - 1`, host and device streams: the call returns 0 with a
    message.  Fixed rate: before any GPU work, the whole buffer stays the
    prefill.  Variable rate: nothing at or past the capacity and nothing before
    the stream changes.  The same thread then compresses the field with enough
    capacity and gets the reference stream: the lease and the context are usable."""
    dtype = np.dtype(dtype)
    ztype = TYPES[dtype]
    params = _params(mode, param, ztype, dims)
    fixed = params[0] == params[1]
    shape = SHAPES[dims][1]
    a = _field(dtype, shape, mode == "reversible")
    job = _dense_job(shape, ztype, params)
    rng = np.random.default_rng(5)
    for dev in (False, True):
        fptr = _device_field(a).data_ptr() if dev else a.ctypes.data
        for off in (0, 63, 100):
            ref = _ref(request, a, mode, param, off)
            head = head_bits_for(rng, off)
            buf = Buffer(ref.exact - 1, dev)
            rc, _ = _compress(hip, job, fptr, buf, ref.exact - 1, off, head)
            assert rc == 0 and hip.zfp_hip_last_error(), (dev, off)
            _check_refused(buf, off, strict=fixed)
            buf = Buffer(ref.exact, dev)
            rc, end = _compress(hip, job, fptr, buf, ref.exact, off, head)
            assert rc == 1, (dev, off, hip.zfp_hip_last_error().decode())
            assert end == ref.end_bit
            buf.check(off, head, ref.words, end, (dev, off, "after a refusal"))


# ---------------------------------------------------------------------------
# decode is a function of the stream's bits
DECODE = [_case("f4", 3, "rate", 1), _case("f4", 3, "rate", 3.25), _case("f8", 3, "precision", 20),
          _case("f4", 3, "reversible", None), _case("f4", 4, "rate", 3.25), _case("f4", 4, "reversible", None)]
DECODE += [_case(t, d, m, p) for t in ("f4", "i4") for d in (1, 2)
           for m, p in (("rate", 12), ("precision", 18 if t == "f4" else 14))]


def _tails(ref, bit_offset, rng):
    """The reference stream in three surroundings: (name, capacity, words from
    word 0).  Below the offset: pattern words and random pending bits."""
    base = ref.words[:ref.exact].copy()
    lead = streams.pattern(ref.exact)
    w0, g0 = bit_offset // 64, bit_offset % 64
    base[:w0] = lead[:w0]
    base[w0] |= np.uint64(head_bits_for(rng, bit_offset))
    dirty = np.concatenate([base, streams.pattern(2, first=ref.exact)])
    if ref.end_bit % 64:  # the unused high bits of the last word: another stream's, not zero
        dirty[ref.exact - 1] |= lead[ref.exact - 1] & np.uint64(((1 << 64) - 1) << (ref.end_bit % 64) & ((1 << 64) - 1))
    return [("exact", ref.exact, base), ("zeros", ref.exact + 2, np.concatenate([base, np.zeros(2, dtype=np.uint64)])),
            ("pattern", ref.exact + 2, dirty)]


@pytest.mark.parametrize("dtype,dims,mode,param,env", DECODE)
def test_decode_depends_on_the_stream_bits_only(hip, request, monkeypatch, dtype, dims, mode, param, env):
    """The reference stream at bit offsets 0, 63 and 100, decoded with a capacity
    of exactly its words, with two zero words after it and with pattern words
    after it (pattern in the unused bits of its last word too), from host and
    device memory: every output is the reference decode.  Variable rate: with
    the encoder's index, with the scan, and with the scan in 64-bit segments --
    the block starts found do not depend on what follows the last block."""
    dtype = np.dtype(dtype)
    ztype = TYPES[dtype]
    params = _params(mode, param, ztype, dims)
    fixed = params[0] == params[1]
    # (reversible streams are long and the 64-bit-segment scan takes a pass per
    # segment: the smaller shape, still more than one wave of blocks)
    shape = SHAPES[dims][0 if mode == "reversible" else 1]
    a = _field(dtype, shape, mode == "reversible")
    job = _dense_job(shape, ztype, params)
    rng = np.random.default_rng(9)
    index = None if fixed else hip.zfp_hip_index_create()
    try:
        for off in (0, 63, 100):
            ref = _ref(request, a, mode, param, off)
            end_bit = ref.end_bit
            if not fixed:  # the encoder's index for this offset (its stream is checked against the reference)
                buf = Buffer(ref.exact, True)
                rc, end = _compress(hip, job, _device_field(a).data_ptr(), buf, ref.exact, off, 0, index)
                assert rc == 1, hip.zfp_hip_last_error().decode()
                assert end == end_bit
                buf.check(off, 0, ref.words, end_bit, (off, "stream for the index"))
            variants = [("fixed", None, None)] if fixed else [("index", index, None), ("scan", None, None),
                                                              ("scan64", None, "64")]
            for tail, cap, words in _tails(ref, off, rng):
                for dev in (False, True):
                    buf = Buffer(cap, dev, fill=words)
                    for vname, idx, seg in variants:
                        if seg:
                            monkeypatch.setenv("ZFP_HIP_SCAN_SEG_BITS", seg)
                        else:
                            monkeypatch.delenv("ZFP_HIP_SCAN_SEG_BITS", raising=False)
                        what = (off, tail, "device" if dev else "host", vname)
                        rc, dend, got = _decompress(hip, job, a, dev, buf.ptr, cap, off, idx)
                        assert rc == 1, (what, hip.zfp_hip_last_error().decode())
                        if not fixed:
                            assert _scanned(hip) == (idx is None), (what, "scan")
                        assert dend == end_bit, what
                        assert got == ref.decoded.tobytes(), what
                    assert (buf.read() == buf.prefill).all(), (off, tail, dev, "a decode wrote to the stream")
    finally:
        monkeypatch.delenv("ZFP_HIP_SCAN_SEG_BITS", raising=False)
        if index:
            hip.zfp_hip_index_free(index)


# ---------------------------------------------------------------------------
# through the C API
def _capi_field(api, a, dev):
    if not dev:
        return api.field_for(a)
    make = {2: api.lib.zfp_field_2d, 3: api.lib.zfp_field_3d}[a.ndim]
    return make(ctypes.c_void_p(_device_field(a).data_ptr()), TYPES[a.dtype], *reversed(a.shape))


@pytest.mark.parametrize("lead", ["header", "pad100"])
@pytest.mark.parametrize("dtype,dims,mode,param,env", [_case("f4", 3, "rate", 8), _case("f4", 3, "precision", 20),
                                                       _case("i4", 2, "rate", 12)])
def test_c_api_on_dirty_buffers(product, ref_capi, dtype, dims, mode, param, env, lead):
    """stream_open on a pattern-filled host or device buffer, zfp_write_header or
    stream_pad(100), zfp_compress: the whole buffer is the reference's bytes
    (header included) inside the prefill, the return value is the reference's
    and stream_wtell is at the flushed word boundary."""
    dtype = np.dtype(dtype)
    ztype = TYPES[dtype]
    shape = SHAPES[dims][1]
    a = _field(dtype, shape)
    kw = {"header": True} if lead == "header" else {"pad_bits": 100}
    want = ref_capi.compress(a, mode, param, ztype=ztype, **kw)
    assert len(want) % 8 == 0
    ref_words = streams.as_words(want)
    cap = _max_words(product, shape, ztype, mode, param) + 8
    for dev in (False, True):
        buf = Buffer(cap, dev)
        field = _capi_field(product, a, dev)
        n, at = streams.capi_compress_into(product, field, dims, mode, param, ztype, buf.ptr, 8 * cap, **kw)
        product.lib.zfp_field_free(field)
        assert n == len(want), (dev, product.lib.zfp_hip_last_error())
        assert at == 8 * n, (dev, "stream_wtell")
        # the leading bits were written by the host bitstream: everything from bit 0 is the reference's
        buf.check(0, 0, ref_words, 8 * len(want), ("device" if dev else "host", lead))


def test_c_api_refuses_a_short_buffer(product, oracle):
    """zfp_compress on a stream_open of `exact` words less one returns 0, and a
    stream of `exact` words takes the reference stream."""
    shape = SHAPES[3][0]
    a = _field(np.float32, shape)
    words, end = oracle.compress_words(a, params_rate(8, 3, 3))
    exact = exact_words(end)
    for nbytes in (8 * exact - 8, 8 * exact):
        buf = Buffer(exact, False)
        field = product.field_for(a)
        n, _ = streams.capi_compress_into(product, field, 3, "rate", 8, 3, buf.ptr, nbytes)
        product.lib.zfp_field_free(field)
        if nbytes < 8 * exact:
            assert n == 0
            assert (buf.read() == buf.prefill).all()
        else:
            assert n == 8 * exact
            buf.check(0, 0, words, end, "exact")
