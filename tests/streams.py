"""Stream buffers for the buffer-edge tests (test infrastructure only).

The contract pinned here is the reference's: zfp_compress writes the bits from
the current position through the zero-padded last word and touches nothing
else; the bits below the start position in the start word are the bitstream's
pending bits (the `head_word` argument of zfp_hip_compress), not what memory
holds.  expected_image() builds that result from a prefilled buffer and a
reference stream; Buffer is a host or device allocation prefilled with a
position-dependent pattern, with GUARD words before word 0 of the stream and
GUARD words beyond its capacity, so "past the capacity" and "inside the
capacity but past the stream" are separate checks.

Word and bit positions are absolute in the stream (word 0 is the word the
`words` argument points at); reference streams are given the same way (the
oracle's compress_words(bit_offset=...) and the reference library after
stream_pad both leave zeros below the offset).
"""
import ctypes

import numpy as np

GUARD = 4
PATTERN = 0x9E3779B97F4A7C15
REGIONS = ("before the stream", "pending bits of the start word", "stream bits", "zero padding of the last word",
           "after the stream, inside the capacity", "past the capacity")


def pattern(n, first=0):
    """Words first .. first+n-1 of the prefill: (i + 1) * PATTERN mod 2^64, never zero."""
    return (np.arange(first + 1, first + n + 1, dtype=np.uint64) * np.uint64(PATTERN)).astype(np.uint64)


def bits_of(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")


def words_of(bits):
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def as_words(data):
    """Bytes of a C API stream (a whole number of words) as uint64 words."""
    data = bytes(data)
    return np.frombuffer(data + bytes((-len(data)) % 8), dtype=np.uint64).copy()


def exact_words(end_bit):
    """The smallest capacity, in words from the buffer start, that holds a stream ending at end_bit."""
    return (end_bit + 63) // 64


def expected_image(prefill_words, bit_offset, head_bits, ref_words, end_bit):
    """What an encode from bit_offset to end_bit leaves in a buffer that held
    prefill_words (word 0 = the stream's word 0):

      words below bit_offset // 64                    unchanged
      the low bit_offset % 64 bits of that word       head_bits (not memory)
      bits [bit_offset, end_bit)                      ref_words' bits
      bits [end_bit, roundup64(end_bit))              zero
      every later word                                unchanged
    """
    out = np.array(prefill_words, dtype=np.uint64, copy=True)
    w0, g0 = bit_offset // 64, bit_offset % 64
    w1 = exact_words(end_bit)
    assert bit_offset < end_bit and w1 <= len(out) and len(ref_words) >= w1
    bits = bits_of(np.asarray(ref_words, dtype=np.uint64)[w0:w1])
    bits[:g0] = bits_of(np.array([head_bits], dtype=np.uint64))[:g0]
    bits[end_bit - 64 * w0:] = 0
    out[w0:w1] = words_of(bits)
    return out


def region_of(bit, bit_offset, end_bit, capacity_words):
    """Which of REGIONS the absolute stream bit position `bit` (negative: the leading guard) lies in."""
    if bit < bit_offset // 64 * 64:
        return REGIONS[0]
    if bit < bit_offset:
        return REGIONS[1]
    if bit < end_bit:
        return REGIONS[2]
    if bit < exact_words(end_bit) * 64:
        return REGIONS[3]
    if bit < capacity_words * 64:
        return REGIONS[4]
    return REGIONS[5]


def difference(got, want, bit_offset, end_bit, capacity_words, lead=GUARD):
    """None when the two whole allocations (`lead` guard words before word 0)
    are equal, else a description of the first differing word."""
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    if not bad.size:
        return None
    i = int(bad[0])
    x = int(got[i] ^ want[i])
    low = (x & -x).bit_length() - 1
    w = i - lead
    return ("word %d of the stream differs (%d words differ, last %d): got %016x, expected %016x, first bit %d: %s"
            % (w, bad.size, int(bad[-1]) - lead, int(got[i]), int(want[i]), 64 * w + low,
               region_of(64 * w + low, bit_offset, end_bit, capacity_words)))


class Buffer:
    """GUARD + capacity_words + GUARD pattern words in host (numpy) or device
    (torch) memory; `ptr` is the address of word 0 of the stream.  `fill`: the
    words from word 0 on are taken from it (a stream to decode) where given."""

    def __init__(self, capacity_words, device, fill=None):
        self.capacity = capacity_words
        self.prefill = pattern(GUARD + capacity_words + GUARD)
        if fill is not None:
            self.prefill[GUARD:GUARD + len(fill)] = fill
        self.device = device
        if device:
            import torch
            self.mem = torch.from_numpy(self.prefill.view(np.int64).copy()).cuda()
            self.ptr = self.mem.data_ptr() + 8 * GUARD
        else:
            self.mem = self.prefill.copy()
            self.ptr = self.mem.ctypes.data + 8 * GUARD

    def read(self):
        """The whole allocation as it is now."""
        if self.device:
            import torch
            torch.cuda.synchronize()
            return self.mem.cpu().numpy().view(np.uint64)
        return self.mem.copy()

    def expect(self, bit_offset, head_bits, ref_words, end_bit):
        """The whole allocation after an encode (expected_image behind the leading guard)."""
        want = self.prefill.copy()
        want[GUARD:] = expected_image(self.prefill[GUARD:], bit_offset, head_bits, ref_words, end_bit)
        return want

    def check(self, bit_offset, head_bits, ref_words, end_bit, what):
        msg = difference(self.read(), self.expect(bit_offset, head_bits, ref_words, end_bit), bit_offset, end_bit,
                         self.capacity)
        assert msg is None, (what, msg)


def head_bits_for(rng, bit_offset):
    """Random pending bits below bit_offset % 64 (zero above)."""
    g0 = bit_offset % 64
    return int(rng.integers(0, 1 << 63, dtype=np.uint64)) & ((1 << g0) - 1) if g0 else 0


def capi_compress_into(api, field, ndim, mode, param, ztype, ptr, nbytes, header=False, pad_bits=0, lead_bits=()):
    """The C API call sequence on a caller's buffer (host or device memory, not
    zeroed) for the zfp_field `field`: stream_open(ptr, nbytes), optionally
    zfp_write_header or stream_pad(pad_bits) or stream_write_bits for every
    (value, nbits) of lead_bits, then zfp_compress.  Returns (zfp_compress's
    return value, stream_wtell after it)."""
    lib = api.lib
    zs = lib.zfp_stream_open(None)
    api.set_mode(zs, mode, param, ztype, ndim)
    bs = lib.stream_open(ctypes.c_void_p(ptr), nbytes)
    lib.zfp_stream_set_bit_stream(zs, bs)
    lib.zfp_stream_rewind(zs)
    if header:
        assert lib.zfp_write_header(zs, field, 7)
    if pad_bits:
        lib.stream_pad(bs, pad_bits)
    for value, nbits in lead_bits:
        lib.stream_write_bits(bs, value, nbits)
    n = lib.zfp_compress(zs, field)
    at = lib.stream_wtell(bs)
    lib.stream_close(bs)
    lib.zfp_stream_close(zs)
    return n, at
