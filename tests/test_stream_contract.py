"""The stream buffer contract, pinned on the reference library (no GPU).

zfp_compress writes the bits from the current position through the
zero-padded last word and touches nothing else; the bits below the start
position are the bitstream's pending bits.  streams.expected_image states
that, and test_gpu_stream_edges.py holds the HIP codec to it.  Here the
reference library itself writes into a pattern-filled host buffer through the
C API and must leave exactly expected_image built from the oracle's stream,
which shows that the contract is the reference's and checks the helper.
"""
import numpy as np
import pytest

import layouts
import streams
from pyoracle import params_precision, params_rate, params_reversible
from streams import GUARD, Buffer, exact_words, expected_image


def test_expected_image_regions():
    pre = streams.pattern(6)
    assert (pre != 0).all() and len(set(pre.tolist())) == 6
    ref = np.array([0, ~np.uint64(0), ~np.uint64(0), 0, 0, 0], dtype=np.uint64)
    head = 0x155
    img = expected_image(pre, 64 + 10, head, ref, 128 + 7)
    assert img[0] == pre[0]                                   # below the start word
    assert int(img[1]) == (((1 << 64) - 1) & ~0x3ff) | head   # pending bits, then stream bits
    assert int(img[2]) == 0x7f                                # stream bits, then zero padding
    assert (img[3:] == pre[3:]).all()                         # later words
    names = [streams.region_of(b, 74, 135, 4) for b in (-1, 63, 64, 73, 74, 134, 135, 191, 192, 255, 256)]
    assert names == [streams.REGIONS[i] for i in (0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5)]
    got = np.concatenate([streams.pattern(GUARD), img])
    want = got.copy()
    assert streams.difference(got, want, 74, 135, 4) is None
    got[GUARD + 3] ^= np.uint64(1 << 5)
    msg = streams.difference(got, want, 74, 135, 4)
    assert "word 3 " in msg and "first bit 197" in msg and streams.REGIONS[4] in msg


@pytest.mark.parametrize("shape,dtype,mode,param,params,offset", [
    ((8, 12, 68), np.float32, "rate", 3.25, params_rate(3.25, 3, 3), 0),
    ((13, 22), np.float64, "reversible", None, params_reversible(), 63),
    ((9, 6, 10, 13), np.float32, "precision", 20, params_precision(20), 100),
])
def test_reference_library_leaves_the_expected_image(ref_capi, oracle, shape, dtype, mode, param, params, offset):
    """Offset 0: nothing before the stream.  Offset 63: 63 random bits written
    with stream_write_bits are pending when zfp_compress starts (the head bits).
    Offset 100: stream_pad, whose first word reaches memory before the call."""
    rng = np.random.default_rng(offset)
    a = layouts.special_field(shape, dtype, rng)
    words, end = oracle.compress_words(a, params, bit_offset=offset)
    cap = exact_words(end) + 3
    buf = Buffer(cap, False)
    head = streams.head_bits_for(rng, offset) if offset == 63 else 0
    kw = {"lead_bits": [(head, 63)]} if offset == 63 else {"pad_bits": offset} if offset else {}
    field = ref_capi.field_for(a)
    n, at = streams.capi_compress_into(ref_capi, field, a.ndim, mode, param, 3 if dtype == np.float32 else 4, buf.ptr,
                                       8 * cap, **kw)
    ref_capi.lib.zfp_field_free(field)
    assert n == 8 * exact_words(end) and at == 8 * n
    if offset == 100:  # stream_pad flushed word 0 (zeros) itself; the pending bits of word 1 are zeros too
        buf.prefill[GUARD] = 0
    buf.check(offset, head, words, end, (shape, mode, offset))
