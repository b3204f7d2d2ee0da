"""A catalogue of small library calls with CPU-made expected results, and the
tools that run them in sequences (test infrastructure only, no pytest marks).

Every zfp_hip_* call borrows a device context from a process-wide pool and
inherits what the previous call on it left behind: look-back status words,
staging buffers that only grow, the scan's index and its cached start table,
pinned staging, the side streams of the slab pipeline.  The catalogue exists so
that the same calls can be made in every order on one context
(test_gpu_call_sequences.py) and from eight threads at once
(test_gpu_concurrent_calls.py), each call checked on its own.

An Entry has three parts:

  prepare(oracle, ref_capi)   CPU only: the inputs and the expected result
                              (float and double from the oracle, integer fields
                              from the reference library, refused calls against
                              the prefill -- nothing from the product)
  setup(hip, product)         once per test, outside the sequences: uploads of
                              read-only device inputs, indices of streams
  run(hip, product, slot)     the call and every assertion on its result; `slot`
                              holds the caller's private mutable buffers, so
                              eight threads can run one entry at once.  Read-only
                              inputs (entry.state, entry.gpu) are shared.

Encodes write into a dirty streams.Buffer and compare the whole allocation;
decodes write into a sentinel-filled destination with guard bands and compare
the whole allocation.  Every entry then asserts the per-thread status it
implies (zfp_hip_last_scan, zfp_hip_last_stale_index, the slab pipeline's
timing signature, zfp_hip_last_error after a refusal).

An entry with `env` (ZFP_HIP_SLOT_WORDS, ZFP_HIP_OVF_POOL) sets and restores it
around its own call when slot.set_env is true -- legal in single-threaded tests
only; every knob is read with getenv per call.  The expected result does not
depend on it: the knobs pick the path, not the stream.
"""
import contextlib
import ctypes
import os
import random
import zlib

import numpy as np

import layouts
import streams
from pyoracle import max_block_bits
from streams import Buffer, exact_words, head_bits_for
from test_block_api import _block_fns
from test_blocks_api import _mask_bw
from test_gpu_boxes import _table
from test_gpu_region import LIB_HIP, SENTINEL, TYPES, _arr4, _blocks, _guarded, _job, _params, _region_decode
from test_gpu_region_encode import _classify, _splice
from test_gpu_stream_edges import (PIPE, PIPE_SHAPE, REDO3, REDO4, SHAPES, SLOTS3, SLOTS4, Ref, _check_refused,
                                   _compress, _dense_job, _nblocks, _pipelined, _ref_end_bit)

FAKE_DEVICE = False  # the CPU stub test: "device" memory is host memory
DEST_GUARD = 16      # elements before and after a dense decode destination


def bind(lib):
    """Argument types of every libzfp_hip.so entry the catalogue calls."""
    vp, u64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    for name, res, args in [
            ("zfp_hip_compress", ci, [vp, vp, vp, u64, u64, u64, ci, vp, vp]),
            ("zfp_hip_decompress", ci, [vp, vp, vp, u64, u64, ci, vp, vp]),
            ("zfp_hip_decompress_region", ci, [vp, vp, vp, vp, vp, vp, u64, u64, ci, vp, vp]),
            ("zfp_hip_decompress_regions", ci, [vp, vp, u64, vp, u64, u64, ci, vp, vp]),
            ("zfp_hip_compress_region", ci, [vp, vp, vp, vp, vp, vp, u64, u64, ci, vp]),
            ("zfp_hip_index_build", ci, [vp, vp, u64, u64, ci, vp]),
            ("zfp_hip_index_create", vp, []), ("zfp_hip_index_free", None, [vp]),
            ("zfp_hip_index_export", ctypes.c_size_t, [vp, vp, ctypes.c_size_t]),
            ("zfp_hip_index_import", vp, [vp, ctypes.c_size_t]),
            ("zfp_hip_last_error", ctypes.c_char_p, []), ("zfp_hip_last_scan", ci, [vp, vp]),
            ("zfp_hip_last_timing", ci, [vp, vp]), ("zfp_hip_last_stale_index", ci, []),
            ("zfp_hip_release_scratch", ci, [])]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def load():
    return bind(ctypes.CDLL(LIB_HIP))


# ---------------------------------------------------------------------------
# memory
class DevArray:
    """A numpy array's bytes in device memory (host memory under FAKE_DEVICE)."""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.dtype, self.shape = a.dtype, a.shape
        if FAKE_DEVICE:
            self.mem = a.copy()
            self.ptr = self.mem.ctypes.data
        else:
            import torch
            self.mem = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
            self.ptr = self.mem.data_ptr()

    def get(self):
        if FAKE_DEVICE:
            return self.mem.copy()
        import torch
        torch.cuda.synchronize()
        return self.mem.cpu().numpy().view(self.dtype).reshape(self.shape)


def _buffer(capacity, device, fill=None):
    return Buffer(capacity, device and not FAKE_DEVICE, fill)


class Dest:
    """A dense decode destination inside DEST_GUARD sentinel elements on either
    side, in host or device memory; check() compares the whole allocation."""

    def __init__(self, shape, dtype, device):
        self.n = int(np.prod(shape))
        self.big = np.empty(self.n + 2 * DEST_GUARD, dtype=dtype)
        self.big.view(np.uint8)[...] = SENTINEL
        self.dev = DevArray(self.big) if device else None
        self.ptr = (self.dev.ptr if device else self.big.ctypes.data) + DEST_GUARD * self.big.itemsize

    def check(self, want, what):
        got = self.dev.get() if self.dev else self.big
        expect = np.empty_like(self.big)
        expect.view(np.uint8)[...] = SENTINEL
        if want is not None:
            expect[DEST_GUARD:DEST_GUARD + self.n] = np.ascontiguousarray(want).reshape(-1)
        if got.tobytes() != expect.tobytes():
            bad = np.nonzero(got.view(layouts.uint_of(got.dtype)) != expect.view(layouts.uint_of(got.dtype)))[0]
            raise AssertionError("%s: destination differs in %d elements, first at %d (guard: %d elements each side)"
                                 % (what, bad.size, int(bad[0]) - DEST_GUARD, DEST_GUARD))


class Slot:
    """One caller's private mutable buffers.  set_env: the entry may change the
    environment around its call (single-threaded tests only).  index_for: per
    entry name, an index to use instead of the entry's shared one."""

    def __init__(self, set_env):
        self.set_env = set_env
        self.store = {}
        self.indices = []
        self.index_for = {}
        self.capi = None

    def index(self, hip, key):
        if ("index", key) not in self.store:
            self.store[("index", key)] = hip.zfp_hip_index_create()
            self.indices.append(self.store[("index", key)])
        return self.store[("index", key)]

    def host_words(self, key, nwords):
        """One host word array per key: the same address for every entry of a group."""
        if ("words", key) not in self.store:
            self.store[("words", key)] = np.empty(nwords, dtype=np.uint64)
        assert len(self.store[("words", key)]) >= nwords
        return self.store[("words", key)]

    def close(self, hip):
        for idx in self.indices:
            hip.zfp_hip_index_free(idx)
        self.indices = []
        self.store = {}


@contextlib.contextmanager
def _env(slot, env):
    if not (slot.set_env and env):
        yield
        return
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------
# fields and references
def field(dtype, shape, tag="", rev=False):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(zlib.crc32(repr((dtype.name, shape, tag)).encode()))
    if dtype.kind == "i":
        a = layouts.edge_ints(shape, dtype, rng, full_range=rev)
    else:
        a = layouts.special_field(shape, dtype, rng)
    a.setflags(write=False)
    return a


def reference(oracle, ref_capi, a, mode, param, bit_offset):
    """streams Ref of `a` at a bit offset: the oracle's for floats, the reference
    library's for integers (as test_gpu_stream_edges._ref)."""
    ztype = TYPES[a.dtype]
    params = _params(mode, param, ztype, a.ndim)
    if a.dtype.kind == "f":
        words, end = oracle.compress_words(a, params, bit_offset=bit_offset)
        dec, dend = oracle.decompress_words(words, a.shape, a.dtype, params, bit_offset=bit_offset)
        assert dend == end
    else:
        data = ref_capi.compress(np.array(a), mode, param, ztype=ztype, pad_bits=bit_offset)
        words = streams.as_words(data)
        dec, n = ref_capi.decompress(data, a.shape, a.dtype, mode, param, ztype=ztype, pad_bits=bit_offset)
        assert n == len(data)
        if params[0] == params[1]:
            end = bit_offset + _nblocks(a.shape) * params[1]
        else:
            end = _ref_end_bit(ref_capi, a, mode, param, bit_offset, len(words))
        assert exact_words(end) == len(words)
    return Ref(words, end, dec)


def stream_image(ref, bit_offset, seed, tail=2):
    """The reference stream as a decoder's input: pattern words and random
    pending bits below the offset, pattern in the unused bits of the last word
    and `tail` pattern words after it (a decode depends on the stream's bits only)."""
    rng = np.random.default_rng(seed)
    base = ref.words[:ref.exact].copy()
    lead = streams.pattern(ref.exact)
    w0 = bit_offset // 64
    base[:w0] = lead[:w0]
    base[w0] |= np.uint64(head_bits_for(rng, bit_offset))
    if ref.end_bit % 64:
        base[ref.exact - 1] |= lead[ref.exact - 1] & np.uint64(((1 << 64) - 1) << (ref.end_bit % 64) & ((1 << 64) - 1))
    return np.concatenate([base, streams.pattern(tail, first=ref.exact)])


def _worst_words(shape, ztype, params, bit_offset):
    return (bit_offset + _nblocks(shape) * max_block_bits(params, ztype, len(shape))) // 64 + 8


def slot_dims(dtype, dims, fixed, maxprec, encodes, decodes):
    """The dimensionality of the kernel that ZFP_HIP_SLOT_WORDS applies to in a
    call of this kind (host_launch.h: short_slot_words, short_slot_words4,
    short_stage_words), or None when the call reads no such knob."""
    dtype = np.dtype(dtype)
    if fixed or dtype.kind != "f":
        return None
    if encodes and dims == 3:
        return 3
    if encodes and dims == 4 and dtype.itemsize == 4:
        return 4
    if decodes and dims == 3 and dtype.itemsize == 8 and maxprec <= 32:
        return 3
    return None


# ---------------------------------------------------------------------------
class Entry:
    def __init__(self, name, kind, prepare, run, setup=None, env=None, scans=False, stale=False, fails=None,
                 pipelined=False, slot_dims=None):
        self.name, self.kind = name, kind
        self._prepare, self._run, self._setup = prepare, run, setup
        self.env = env
        self.scans, self.stale, self.fails, self.pipelined = scans, stale, fails, pipelined
        self.slot_dims = slot_dims
        self.state = None
        self.gpu = {}

    def prepare(self, oracle, ref_capi):
        if self.state is None:
            self.state = self._prepare(oracle, ref_capi)
        return self.state

    def setup(self, hip, product):
        self.teardown(hip)
        if self._setup:
            self._setup(self, hip, product)

    def teardown(self, hip):
        for idx in self.gpu.get("indices", []):
            hip.zfp_hip_index_free(idx)
        self.gpu = {}

    def run(self, hip, product, slot):
        self._run(self, hip, product, slot)

    def __repr__(self):
        return "<%s>" % self.name


def check_status(hip, e, what=None):
    """The per-thread status the entry implies, right after its call."""
    what = what or e.name
    scanned = hip.zfp_hip_last_scan(None, None) != 0
    if scanned != e.scans:
        raise AssertionError("%s: zfp_hip_last_scan says %s, the call %s" % (what, scanned, "scans" if e.scans else
                                                                              "does not scan"))
    stale = hip.zfp_hip_last_stale_index()
    if stale != (1 if e.stale else 0):
        raise AssertionError("%s: zfp_hip_last_stale_index() == %d" % (what, stale))
    if _pipelined(hip) != e.pipelined:
        raise AssertionError("%s: the call %s the slab pipeline" % (what, "did not take" if e.pipelined else "took"))
    if e.fails:
        err = hip.zfp_hip_last_error().decode()
        if not err or not all(s in err for s in e.fails):
            raise AssertionError("%s: zfp_hip_last_error() is %r, expected it to name %r" % (what, err, e.fails))


def _err(hip):
    return hip.zfp_hip_last_error().decode()


# ---- encode ----
def _encode_entry(name, dtype, shape, mode, param, dev_field, dev_stream, off, cap_extra, index=False, env=None,
                  pipelined=False, group=None):
    dtype = np.dtype(dtype)
    ztype, dims = TYPES[dtype], len(shape)
    params = _params(mode, param, ztype, dims)
    fixed = params[0] == params[1]

    def prepare(oracle, ref_capi):
        a = field(dtype, shape, name, mode == "reversible")
        ref = reference(oracle, ref_capi, a, mode, param, off)
        head = head_bits_for(np.random.default_rng(zlib.crc32(name.encode())), off)
        return dict(a=a, ref=ref, job=_dense_job(shape, ztype, params), off=off, head=head, cap=ref.exact + cap_extra,
                    mode=mode, param=param, fixed=fixed)

    def setup(e, hip, product):
        if dev_field:
            e.gpu["field"] = DevArray(e.state["a"])

    def run(e, hip, product, slot):
        st = e.state
        ref, cap = st["ref"], st["cap"]
        fptr = e.gpu["field"].ptr if dev_field else st["a"].ctypes.data
        if group:  # the same stream address for every entry of the group
            arr = slot.host_words(group, _worst_words(shape, ztype, params, off) + 2 * streams.GUARD)
            buf = Buffer.__new__(Buffer)
            buf.capacity, buf.device = cap, False
            buf.prefill = streams.pattern(2 * streams.GUARD + cap)
            buf.mem = arr[:2 * streams.GUARD + cap]
            buf.mem[...] = buf.prefill
            buf.ptr = buf.mem.ctypes.data + 8 * streams.GUARD
        else:
            buf = _buffer(cap, dev_stream)
        idx = slot.index(hip, group or name) if index else None
        with _env(slot, e.env):
            rc, end = _compress(hip, st["job"], fptr, buf, cap, off, st["head"], idx)
        assert rc == 1, (name, _err(hip))
        check_status(hip, e)
        assert end == ref.end_bit, (name, "end_bit", end, ref.end_bit)
        buf.check(off, st["head"], ref.words, end, name)
        if index:  # the index the call filled decodes the stream without a scan
            dest = Dest(shape, dtype, dev_field)
            dend = ctypes.c_uint64(0)
            with _env(slot, e.env):
                rc = hip.zfp_hip_decompress(ctypes.byref(st["job"]), dest.ptr, buf.ptr, cap, off, -1, idx,
                                            ctypes.byref(dend))
            assert rc == 1, (name, "decode with the encoder's index", _err(hip))
            check_status(hip, e, name + " (decode with the encoder's index)")
            assert dend.value == end, (name, "decode end_bit")
            dest.check(ref.decoded, name + " (decode with the encoder's index)")

    return Entry(name, "encode", prepare, run, setup, env=env, pipelined=pipelined,
                 slot_dims=slot_dims(dtype, dims, fixed, params[2], True, index))


# ---- decode ----
def _decode_entry(name, dtype, shape, mode, param, dev, off=0, index=False, pipelined=False, group=None):
    dtype = np.dtype(dtype)
    ztype, dims = TYPES[dtype], len(shape)
    params = _params(mode, param, ztype, dims)
    fixed = params[0] == params[1]

    def prepare(oracle, ref_capi):
        a = field(dtype, shape, name, mode == "reversible")
        ref = reference(oracle, ref_capi, a, mode, param, off)
        words = stream_image(ref, off, zlib.crc32(name.encode()))
        words.setflags(write=False)
        return dict(a=a, ref=ref, job=_dense_job(shape, ztype, params), off=off, words=words, cap=len(words),
                    mode=mode, param=param, fixed=fixed)

    def setup(e, hip, product):
        st = e.state
        if dev:
            e.gpu["words"] = DevArray(st["words"])
        if index:
            idx = hip.zfp_hip_index_create()
            e.gpu["indices"] = [idx]
            wptr = e.gpu["words"].ptr if dev else st["words"].ctypes.data
            rc = hip.zfp_hip_index_build(ctypes.byref(st["job"]), wptr, st["cap"], off, -1, idx)
            assert rc == 1, (name, "zfp_hip_index_build", _err(hip))

    def run(e, hip, product, slot):
        st = e.state
        ref = st["ref"]
        if dev:
            wptr = e.gpu["words"].ptr
        elif group:  # one reused host buffer: the same pointer, other contents
            arr = slot.host_words(group, _worst_words(shape, ztype, params, off) + 2)
            arr[...] = streams.pattern(len(arr), first=7)
            arr[:st["cap"]] = st["words"]
            wptr = arr.ctypes.data
        else:
            wptr = st["words"].ctypes.data
        idx = slot.index_for.get(name, e.gpu["indices"][0]) if index else None
        dest = Dest(shape, dtype, dev)
        end = ctypes.c_uint64(0)
        rc = hip.zfp_hip_decompress(ctypes.byref(st["job"]), dest.ptr, wptr, st["cap"], off, -1, idx, ctypes.byref(end))
        assert rc == 1, (name, _err(hip))
        check_status(hip, e)
        assert end.value == ref.end_bit, (name, "end_bit", end.value, ref.end_bit)
        dest.check(ref.decoded, name)

    return Entry(name, "decode", prepare, run, setup, scans=not fixed and not index, pipelined=pipelined,
                 slot_dims=slot_dims(dtype, dims, fixed, params[2], False, True))


def _export(hip, idx):
    n = hip.zfp_hip_index_export(idx, None, 0)
    blob = ctypes.create_string_buffer(n)
    assert hip.zfp_hip_index_export(idx, blob, n) == n
    return bytearray(blob.raw)


def _stale_entry(name, shape, mode, param):
    """Stream B decoded with stream A's index of the same geometry.  A's block
    lengths and bases, under B's bit count and fingerprint so that the sampled
    match test passes (as test_gpu_region.test_index_handling builds it): the
    decode kernels catch the lengths, the call scans and decodes again."""
    dtype = np.dtype(np.float32)
    params = _params(mode, param, 3, 3)

    def prepare(oracle, ref_capi):
        a, b = field(dtype, shape, "stale-A"), field(dtype, shape, "stale-B")
        ra, rb = reference(oracle, ref_capi, a, mode, param, 0), reference(oracle, ref_capi, b, mode, param, 0)
        assert ra.words.tobytes() != rb.words.tobytes()
        return dict(a=b, ref=rb, other=ra, job=_dense_job(shape, 3, params), off=0, fixed=False)

    def setup(e, hip, product):
        st = e.state
        blobs = []
        for r in (st["other"], st["ref"]):
            idx = hip.zfp_hip_index_create()
            rc = hip.zfp_hip_index_build(ctypes.byref(st["job"]), r.words.ctypes.data, r.exact, 0, -1, idx)
            assert rc == 1, (name, "zfp_hip_index_build", _err(hip))
            blobs.append(_export(hip, idx))
            hip.zfp_hip_index_free(idx)
        ea, eb = blobs
        ea[24:32] = eb[24:32]  # total bits
        ea[48:56] = eb[48:56]  # fingerprint
        wrong = hip.zfp_hip_index_import(bytes(ea), len(ea))
        assert wrong, (name, "zfp_hip_index_import")
        e.gpu["indices"] = [wrong]

    def run(e, hip, product, slot):
        st = e.state
        ref = st["ref"]
        dest = Dest(shape, dtype, False)
        end = ctypes.c_uint64(0)
        rc = hip.zfp_hip_decompress(ctypes.byref(st["job"]), dest.ptr, ref.words.ctypes.data, ref.exact, 0, -1,
                                    e.gpu["indices"][0], ctypes.byref(end))
        assert rc == 1, (name, _err(hip))
        check_status(hip, e)
        assert end.value == ref.end_bit, (name, "end_bit")
        dest.check(ref.decoded, name)

    return Entry(name, "decode-stale", prepare, run, setup, scans=True, stale=True)


# ---- region decode ----
REGION_SHAPE = SHAPES[3][1]
REGION_BOX = ((3, 17), (5, 22), (6, 127))  # unaligned on both ends of every axis
BATCH = [((3, 17), (5, 22), (6, 127)),     # 5 regions: one repeated, one overlapping
         ((0, 4), (0, 4), (0, 4)),
         ((3, 17), (5, 22), (6, 127)),
         ((9, 18), (11, 23), (64, 130)),
         ((17, 18), (0, 23), (129, 130))]


def _region_prepare(mode, param, name):
    params = _params(mode, param, 3, 3)

    def prepare(oracle, ref_capi):
        a = field(np.float32, REGION_SHAPE, name)
        ref = reference(oracle, ref_capi, a, mode, param, 0)
        words = ref.words[:ref.exact].copy()
        words.setflags(write=False)
        return dict(a=a, ref=ref, words=words, job=_job(REGION_SHAPE, 3, params), params=params,
                    fixed=params[0] == params[1])
    return prepare, params


def _region_views(regions, dev):
    """[(big, view, device copy or None, pointer of the view's first element)]"""
    out = []
    for region in regions:
        big, view = _guarded([hi - lo for lo, hi in region], np.float32)
        d = DevArray(big) if dev else None
        ptr = (d.ptr + (view.ctypes.data - big.ctypes.data)) if dev else view.ctypes.data
        out.append((big, view, d, ptr))
    return out


def _check_region_views(name, regions, views, decoded):
    for i, (region, (big, view, d, _)) in enumerate(zip(regions, views)):
        if d is not None:
            big[...] = d.get()
        want = decoded[tuple(slice(lo, hi) for lo, hi in region)]
        assert np.ascontiguousarray(view).tobytes() == np.ascontiguousarray(want).tobytes(), (name, i, region, "values")
        view.view(np.uint8)[...] = SENTINEL
        assert (big.view(np.uint8) == SENTINEL).all(), (name, i, region, "guard band written")


def _region_entry(name, mode, param, dev, index=False, group=None, batch=False):
    prepare, params = _region_prepare(mode, param, name)
    fixed = params[0] == params[1]
    regions = BATCH if batch else [REGION_BOX]

    def setup(e, hip, product):
        st = e.state
        if dev:
            e.gpu["words"] = DevArray(st["words"])
        if index:
            idx = hip.zfp_hip_index_create()
            e.gpu["indices"] = [idx]
            wptr = e.gpu["words"].ptr if dev else st["words"].ctypes.data
            job = _dense_job(REGION_SHAPE, 3, params)
            assert hip.zfp_hip_index_build(ctypes.byref(job), wptr, len(st["words"]), 0, -1, idx) == 1, (name, _err(hip))

    def run(e, hip, product, slot):
        st = e.state
        nwords = len(st["words"])
        if dev:
            wptr = e.gpu["words"].ptr
        elif group:
            arr = slot.host_words(group, _worst_words(REGION_SHAPE, 3, params, 0) + 2)
            arr[...] = streams.pattern(len(arr), first=11)
            arr[:nwords] = st["words"]
            wptr = arr.ctypes.data
        else:
            wptr = st["words"].ctypes.data
        idx = slot.index_for.get(name, e.gpu["indices"][0]) if index else None
        views = _region_views(regions, dev)
        strides = [[s // 4 for s in view.strides] for _, view, _, _ in views]
        if batch:
            blocks = ctypes.c_uint64(12345)
            rc = hip.zfp_hip_decompress_regions(ctypes.byref(st["job"]), _table(regions, [v[3] for v in views], strides),
                                                len(regions), wptr, nwords, 0, -1, idx, ctypes.byref(blocks))
            assert rc == 1, (name, _err(hip))
            got = blocks.value
        else:
            got = _region_decode(hip, st["job"], regions[0], views[0][3], strides[0], wptr, nwords, 0, idx)
        check_status(hip, e)
        _check_region_views(name, regions, views, st["ref"].decoded)
        assert got == sum(_blocks(r, None, REGION_SHAPE) for r in regions), (name, "blocks_read", got)

    return Entry(name, "regions" if batch else "region", prepare, run, setup, scans=not fixed and not index)


# ---- region encode ----
RENC_SHAPE = SHAPES[3][0]
RENC_BOX = [(1, 7), (2, 11), (5, 63)]


def _region_encode_entry(name, rate, off, dev):
    params = _params("rate", rate, 3, 3)
    maxbits = params[1]

    def prepare(oracle, ref_capi):
        a, new = field(np.float32, RENC_SHAPE, "renc-old"), field(np.float32, RENC_SHAPE, "renc-new")
        new = np.ascontiguousarray(new[tuple(slice(lo, hi) for lo, hi in RENC_BOX)])
        w_old, end = oracle.compress_words(a, params, bit_offset=off)
        img = oracle.decompress_words(w_old, RENC_SHAPE, np.float32, params, bit_offset=off)[0].copy()
        img[tuple(slice(lo, hi) for lo, hi in RENC_BOX)] = new
        w_img, end2 = oracle.compress_words(img, params, bit_offset=off)
        assert end2 == end and len(w_img) == len(w_old)
        cls = _classify(RENC_SHAPE, None, RENC_BOX)
        want = _splice(w_old, w_img, np.nonzero(cls)[0], maxbits, off)
        # the caller's bits below the offset: pattern words and random pending bits, left as they are
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        lead = streams.pattern(len(w_old))
        head = np.uint64(head_bits_for(rng, off))
        for w in (w_old, want):
            w[:off // 64] = lead[:off // 64]
            w[off // 64] |= head
        big, view = _guarded(list(new.shape), np.float32)
        view[...] = new
        return dict(old=w_old, want=want, big=big, view=view, job=_job(RENC_SHAPE, 3, params),
                    nblocks=int((cls != 0).sum()), fixed=True)

    def run(e, hip, product, slot):
        st = e.state
        n = len(st["old"])
        buf = _buffer(n + 2, dev, fill=st["old"])
        view = st["view"]
        blocks = ctypes.c_uint64(0)
        rc = hip.zfp_hip_compress_region(ctypes.byref(st["job"]), _arr4(ctypes.c_uint64, [lo for lo, _ in RENC_BOX]),
                                         _arr4(ctypes.c_uint64, [hi for _, hi in RENC_BOX]), view.ctypes.data,
                                         _arr4(ctypes.c_int64, [s // 4 for s in view.strides]), buf.ptr, n, off, -1,
                                         ctypes.byref(blocks))
        assert rc == 1, (name, _err(hip))
        check_status(hip, e)
        want = buf.prefill.copy()
        want[streams.GUARD:streams.GUARD + n] = st["want"]
        msg = streams.difference(buf.read(), want, off, off + _nblocks(RENC_SHAPE) * maxbits, n + 2)
        assert msg is None, (name, msg)
        assert blocks.value == st["nblocks"], (name, "blocks_written", blocks.value)

    return Entry(name, "region-encode", prepare, run)


# ---- calls that fail ----
def _nonunit_stride_entry(name):
    """Variable-rate decompress into a host array with non-unit x stride: it fails
    in the copy-out, after the decode and the check word's copy were queued."""
    shape, mode, param = SHAPES[3][0], "precision", 16
    params = _params(mode, param, 3, 3)

    def prepare(oracle, ref_capi):
        a = field(np.float32, shape, "nonunit")
        ref = reference(oracle, ref_capi, a, mode, param, 0)
        return dict(a=a, ref=ref, job=_dense_job(shape, 3, params), fixed=False)

    def setup(e, hip, product):
        st = e.state
        idx = hip.zfp_hip_index_create()
        e.gpu["indices"] = [idx]
        rc = hip.zfp_hip_index_build(ctypes.byref(st["job"]), st["ref"].words.ctypes.data, st["ref"].exact, 0, -1, idx)
        assert rc == 1, (name, _err(hip))

    def run(e, hip, product, slot):
        st = e.state
        base = np.empty(shape[::-1], dtype=np.float32)
        base.view(np.uint8)[...] = SENTINEL
        out_t = base.T
        job = _job(shape, 3, params)
        for ax in range(3):
            job.s[ax] = out_t.strides[2 - ax] // 4
        assert job.s[0] != 1
        end = ctypes.c_uint64(0)
        rc = hip.zfp_hip_decompress(ctypes.byref(job), out_t.ctypes.data, st["ref"].words.ctypes.data, st["ref"].exact, 0,
                                    -1, e.gpu["indices"][0], ctypes.byref(end))
        assert rc == 0, (name, "a non-unit x stride was accepted")
        check_status(hip, e)
        assert (base.view(np.uint8) == SENTINEL).all(), (name, "destination written")

    return Entry(name, "fails", prepare, run, setup, fails=("unit x stride",))


def _short_capacity_entry(name):
    """Variable-rate compress at capacity `exact - 1`: refused after the encode,
    before the copy into the caller's stream."""
    shape, mode, param, off = SHAPES[3][1], "precision", 12, 63
    params = _params(mode, param, 3, 3)

    def prepare(oracle, ref_capi):
        a = field(np.float32, shape, "short")
        ref = reference(oracle, ref_capi, a, mode, param, off)
        return dict(a=a, ref=ref, job=_dense_job(shape, 3, params), fixed=False)

    def setup(e, hip, product):
        e.gpu["field"] = DevArray(e.state["a"])

    def run(e, hip, product, slot):
        st = e.state
        cap = st["ref"].exact - 1
        buf = _buffer(cap, True)
        rc, _ = _compress(hip, st["job"], e.gpu["field"].ptr, buf, cap, off, 0x155)
        assert rc == 0, (name, "a stream one word short was accepted")
        check_status(hip, e)
        _check_refused(buf, off, strict=False)

    return Entry(name, "fails", prepare, run, setup, fails=("zfp_hip_compress", "capacity"),
                 slot_dims=slot_dims(np.float32, 3, False, params[2], True, False))


def _region_4d_entry(name):
    """A 4D job handed to a region call: refused before any GPU call."""
    shape = (8, 8, 8, 8)

    def prepare(oracle, ref_capi):
        return dict(job=_job(shape, 3, _params("rate", 8, 3, 4)), fixed=True)

    def run(e, hip, product, slot):
        out = np.full(4096, SENTINEL, dtype=np.uint8)
        words = streams.pattern(4096)
        rc = hip.zfp_hip_decompress_region(ctypes.byref(e.state["job"]), _arr4(ctypes.c_uint64, (0, 0, 0, 0)),
                                           _arr4(ctypes.c_uint64, (4, 4, 4, 4)), out.ctypes.data,
                                           _arr4(ctypes.c_int64, (64, 16, 4, 1)), words.ctypes.data, len(words), 0, -1,
                                           None, None)
        assert rc == 0, (name, "a 4D region was accepted")
        check_status(hip, e)
        assert (out == SENTINEL).all(), (name, "destination written")
        assert (words == streams.pattern(4096)).all(), (name, "stream written")

    return Entry(name, "fails", prepare, run, fails=("zfp_hip_decompress_region", "4D"))


# ---- through libzfp.so ----
def _capi(product, slot):
    """The slot's own binding of libzfp.so: ZfpCAPI keeps the last index on the
    object, which callers on several threads must not share (no index is kept)."""
    if slot.capi is None:
        from capi import ZfpCAPI
        slot.capi = ZfpCAPI(product.path)
    return slot.capi


def _capi_header_entry(name):
    shape, mode, param = SHAPES[3][1], "precision", 16
    params = _params(mode, param, 3, 3)

    def prepare(oracle, ref_capi):
        a = field(np.float32, shape, "capi-header")
        ref = reference(oracle, ref_capi, a, mode, param, 96)
        # the 96 header bits are the reference library's, the blocks the oracle's
        head = ref_capi.compress(np.array(a), mode, param, ztype=3, header=True)[:12]
        want = bytearray(ref.words[:ref.exact].tobytes())
        want[:12] = head
        return dict(a=np.array(a), ref=ref, want=bytes(want), fixed=False)

    def run(e, hip, product, slot):
        st = e.state
        api = _capi(product, slot)
        got = api.compress(st["a"], mode, param, ztype=3, header=True)
        check_status(hip, _NoScan(e), name + " (compress)")
        assert got == st["want"], (name, "stream differs", len(got), len(st["want"]))
        out = np.empty(shape, dtype=np.float32)
        out.view(np.uint8)[...] = SENTINEL
        _, n = api.decompress(st["want"], shape, np.float32, mode, param, ztype=3, header=True, out=out)
        check_status(hip, e)
        assert n == len(st["want"]), (name, "bytes read", n)
        assert out.tobytes() == st["ref"].decoded.tobytes(), (name, "decode")

    return Entry(name, "capi", prepare, run, scans=True, slot_dims=3)


class _NoScan:
    """The status of an entry's non-scanning first call."""

    def __init__(self, e):
        self.name, self.scans, self.stale, self.fails, self.pipelined = e.name, False, False, None, False


def _block_pair_entry(name):
    """One zfp_encode_block / zfp_decode_block pair (pinned staging)."""
    rate = 12
    params = _params("rate", rate, 3, 3)

    def prepare(oracle, ref_capi):
        a = (np.random.default_rng(64).standard_normal((4, 4, 4)) * 100).astype(np.float32)
        a[1, 2, 3], a[3, 0, 1] = 0.0, -1e-3
        words, end = oracle.compress_words(a, params)
        dec, _ = oracle.decompress_words(words, a.shape, np.float32, params)
        return dict(a=a, words=words, end=end, dec=dec, fixed=True)

    def run(e, hip, product, slot):
        st = e.state
        api = _capi(product, slot)
        lib = api.lib
        f = _block_fns(lib, "float", 3)
        zs = lib.zfp_stream_open(None)
        api.set_mode(zs, "rate", rate, 3, 3)
        buf = np.zeros(256, np.uint8)
        bs = lib.stream_open(buf.ctypes.data, buf.size)
        lib.zfp_stream_set_bit_stream(zs, bs)
        lib.zfp_stream_rewind(zs)
        try:
            bits = f["encode"](zs, st["a"].ctypes.data)
            check_status(hip, e, name + " (encode)")
            lib.stream_flush(bs)
            assert bits == st["end"], (name, "bits", bits)
            n = 8 * len(st["words"])
            assert bytes(buf[:n]) == st["words"].tobytes() and not buf[n:].any(), (name, "stream differs")
            lib.zfp_stream_rewind(zs)
            out = np.empty((4, 4, 4), np.float32)
            out.view(np.uint8)[...] = SENTINEL
            used = f["decode"](zs, out.ctypes.data)
            check_status(hip, e, name + " (decode)")
            assert used == st["end"], (name, "bits read", used)
            assert out.tobytes() == st["dec"].tobytes(), (name, "decode")
        finally:
            lib.stream_close(bs)
            lib.zfp_stream_close(zs)

    return Entry(name, "capi", prepare, run)


def _blocks_stream_entry(name):
    """zfp_blocks_compress_single_stream / _decompress_single_stream, 8 parts:
    several chunk calls inside one entry.  The partitioned stream's layout is the
    reference fork's own (the oracle does not write it), so bytes and decode are
    the reference library's, as in test_blocks_api.py."""
    shape, mode, param, nparts = (33, 33, 33), "precision", 32, 8

    def prepare(oracle, ref_capi):
        g = np.indices(shape).sum(axis=0)
        a = (np.sin(0.1 * g) + 0.01 * np.random.default_rng(1).standard_normal(shape)).astype(np.float64)
        cpb = _nblocks(shape) / nparts
        want = ref_capi.blocks_single_stream(a, mode, param, cpb)
        dec = np.zeros_like(a)
        n, meta = ref_capi.blocks_decompress_single_stream(want, dec)
        return dict(a=a, cpb=cpb, want=want, dec=dec, n=n, meta=meta, fixed=False)

    def run(e, hip, product, slot):
        st = e.state
        api = _capi(product, slot)
        got = api.blocks_single_stream(st["a"], mode, param, st["cpb"])
        assert len(got) == len(st["want"]) and _mask_bw(got, 3) == _mask_bw(st["want"], 3), (name, "stream differs")
        out = np.empty(shape, dtype=np.float64)
        out.view(np.uint8)[...] = SENTINEL
        n, meta = api.blocks_decompress_single_stream(st["want"], out)
        check_status(hip, e)
        assert (n, meta) == (st["n"], st["meta"]), (name, "bytes read or header")
        assert out.tobytes() == st["dec"].tobytes(), (name, "decode")

    return Entry(name, "capi", prepare, run, scans=True, slot_dims=3)


# ---------------------------------------------------------------------------
def build_catalogue():
    small3, large3 = SHAPES[3]
    E, D, R = _encode_entry, _decode_entry, _region_entry
    out = [
        # encode
        E("enc-f4-3d-rate16-dev-dev-small", "f4", small3, "rate", 16, True, True, 0, 1),
        E("enc-f4-3d-rate16-dev-dev-large", "f4", large3, "rate", 16, True, True, 0, 1),
        E("enc-f4-3d-rate8-host-host-off64", "f4", large3, "rate", 8, False, False, 64, 2),
        E("enc-f4-3d-rate3.25-dev-dev-off100", "f4", large3, "rate", 3.25, True, True, 100, 2),
        E("enc-f4-3d-prec18-host-index-off1-A", "f4", large3, "precision", 18, False, False, 1, 2, index=True,
          group="enc-prec18"),
        E("enc-f4-3d-prec18-host-index-off1-B", "f4", large3, "precision", 18, False, False, 1, 2, index=True,
          group="enc-prec18"),
        E("enc-f8-3d-prec32-dev-exact-slots", "f8", large3, "precision", 32, True, True, 0, 0, env=SLOTS3),
        E("enc-f8-3d-prec32-dev-exact-redo", "f8", large3, "precision", 32, True, True, 0, 0, env=REDO3),
        E("enc-f4-3d-rev-dev-dev-large", "f4", large3, "reversible", None, True, True, 0, 2),
        E("enc-f4-4d-rev-index-slots", "f4", SHAPES[4][1], "reversible", None, True, True, 0, 2, index=True, env=SLOTS4),
        E("enc-f4-4d-rev-index-redo", "f4", SHAPES[4][1], "reversible", None, True, True, 0, 2, index=True, env=REDO4),
        E("enc-f4-4d-rate3.25", "f4", SHAPES[4][1], "rate", 3.25, True, True, 0, 2),
        E("enc-f8-1d-rate12", "f8", SHAPES[1][1], "rate", 12, False, False, 63, 1),
        E("enc-i4-2d-prec12", "i4", SHAPES[2][1], "precision", 12, True, True, 0, 2),
        E("enc-i8-2d-rev", "i8", SHAPES[2][1], "reversible", None, False, False, 1, 2),
        E("enc-pipe-rate3.25-off100", "f4", PIPE_SHAPE, "rate", 3.25, False, False, 100, 0, pipelined=True),
        E("enc-pipe-prec18-index-off100", "f4", PIPE_SHAPE, "precision", 18, False, False, 100, 0, index=True,
          pipelined=True),
        # decode
        D("dec-f4-3d-rate16-host", "f4", large3, "rate", 16, False),
        D("dec-f4-3d-rate16-dev", "f4", large3, "rate", 16, True),
        D("dec-f4-3d-rate3.25-host", "f4", large3, "rate", 3.25, False, off=63),
        D("dec-f4-3d-rate3.25-dev", "f4", large3, "rate", 3.25, True, off=100),
        D("dec-f4-3d-prec18-index-host", "f4", large3, "precision", 18, False, off=1, index=True),
        D("dec-f4-3d-prec18-index-dev", "f4", large3, "precision", 18, True, index=True),
        D("dec-f4-3d-prec18-scan-A", "f4", large3, "precision", 18, False, group="dec-prec18"),
        D("dec-f4-3d-prec18-scan-B", "f4", large3, "precision", 18, False, group="dec-prec18"),
        D("dec-f8-3d-prec32-scan-dev", "f8", small3, "precision", 32, True, off=63),
        D("dec-f4-4d-rev-index", "f4", SHAPES[4][0], "reversible", None, True, index=True),
        D("dec-f4-4d-rev-scan", "f4", SHAPES[4][0], "reversible", None, False),
        D("dec-f8-1d-rate12", "f8", SHAPES[1][1], "rate", 12, False, off=1),
        D("dec-f4-2d-prec18-scan", "f4", SHAPES[2][1], "precision", 18, True),
        D("dec-i4-2d-prec12-scan", "i4", SHAPES[2][1], "precision", 12, False),
        D("dec-pipe-rate3.25-off100", "f4", PIPE_SHAPE, "rate", 3.25, False, off=100, pipelined=True),
        D("dec-pipe-prec18-index-off100", "f4", PIPE_SHAPE, "precision", 18, False, off=100, index=True, pipelined=True),
        _stale_entry("dec-f4-3d-prec18-stale-index", small3, "precision", 18),
        # region
        R("reg-rate12-host-strided", "rate", 12, False),
        R("reg-rate12-dev-dev", "rate", 12, True),
        R("reg-prec20-caller-index", "precision", 20, False, index=True),
        R("reg-prec20-scan-A", "precision", 20, False, group="reg-prec20"),
        R("reg-prec20-scan-B", "precision", 20, False, group="reg-prec20"),
        R("regs-rate12-dev-dev", "rate", 12, True, batch=True),
        R("regs-prec20-host-scan", "precision", 20, False, batch=True),
        _region_encode_entry("renc-rate8-dev", 8, 0, True),
        _region_encode_entry("renc-rate8-host", 8, 0, False),
        _region_encode_entry("renc-rate3.25-off100-dev", 3.25, 100, True),
        _region_encode_entry("renc-rate3.25-off100-host", 3.25, 100, False),
        # calls that fail
        _nonunit_stride_entry("fail-nonunit-x-stride"),
        _short_capacity_entry("fail-capacity-one-word-short"),
        _region_4d_entry("fail-region-4d"),
        # through libzfp.so
        _capi_header_entry("capi-header-prec16"),
        _block_pair_entry("capi-block-pair"),
        _blocks_stream_entry("capi-blocks-single-stream"),
    ]
    assert len({e.name for e in out}) == len(out)
    return out


_CATALOGUE = None


def catalogue(oracle, ref_capi):
    """The prepared catalogue, built once per process."""
    global _CATALOGUE
    if _CATALOGUE is None:
        entries = build_catalogue()
        for e in entries:
            e.prepare(oracle, ref_capi)
        _CATALOGUE = entries
    return _CATALOGUE


def allowed_in(entry, env):
    """Whether the entry may run under a frozen environment: not when the set's
    ZFP_HIP_SLOT_WORDS would apply to a kernel of another dimensionality than
    the value is meant for (5: 3D, 9: 4D)."""
    words = env.get("ZFP_HIP_SLOT_WORDS")
    if words is None or entry.slot_dims is None:
        return True
    return entry.slot_dims == {"5": 3, "9": 4}[words]


# ---------------------------------------------------------------------------
# sequences
def euler_sequence(n, seed):
    """A closed walk over the complete directed graph on n nodes with
    self-loops: every ordered pair (i, j), (i, i) included, occurs as
    consecutive elements exactly once; n * n + 1 elements.  (Hierholzer's
    algorithm over shuffled edge lists; deterministic per seed.)"""
    rng = random.Random(seed)
    out_edges = []
    for _ in range(n):
        nxt = list(range(n))
        rng.shuffle(nxt)
        out_edges.append(nxt)
    stack, walk = [rng.randrange(n)], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1 and walk[0] == walk[-1]
    return walk


def slices(seq, k):
    """k contiguous pieces of seq, each starting with the last element of the
    previous one, so that no consecutive pair is lost."""
    npairs = len(seq) - 1
    k = max(1, min(k, npairs)) if npairs else 1
    cuts = [npairs * i // k for i in range(k + 1)]
    return [seq[cuts[i]:cuts[i + 1] + 1] for i in range(k)]


def pairs_of(seq):
    return list(zip(seq[:-1], seq[1:]))


class SequenceFailure(AssertionError):
    pass


def run_sequence(entries, seq, call):
    """call(entry) for every element of seq.  The first failure is raised again
    with the failing entry, the three before it and the position."""
    for pos, i in enumerate(seq):
        try:
            call(entries[i])
        except Exception as exc:  # noqa: BLE001 (any failure of the call is the finding)
            before = [entries[j].name for j in seq[max(0, pos - 3):pos]]
            prev = before[-1] if before else "(nothing)"
            raise SequenceFailure("position %d of %d: %s failed after %s (pair %s -> %s): %s: %s"
                                  % (pos, len(seq), entries[i].name, before, prev, entries[i].name,
                                     type(exc).__name__, exc)) from exc
    return set(pairs_of(seq))
