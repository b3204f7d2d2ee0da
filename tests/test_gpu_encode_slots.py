"""The fixed-rate encoders' slot geometry: the compile-time form of
encode3_aligned_full at rate 16 and the run-time forms around it (other rates,
float64, encode3_aligned at rate 16 from an unaligned start and at rate 8 behind
a header), whole stream byte for byte against the oracle.

Field and stream are device resident, so the launcher's choice of kernel
follows from the shape, the rate and the stream start alone:
  64x16x16 rate 16     256 blocks, one workgroup: the smallest launch of the
                       rate-16 kernel
  256x16x16 rate 16    four workgroups, a wave is one x-row
  256x16x16 rate 12/20 12 and 20 words per block: the run-time full kernel
  256x16x16 rate 16 float64
                       never the float kernel's compile-time form
  256x16x16 rate 16, stream opened 8 bytes into the buffer
                       the start is not 16-byte aligned: encode3_aligned
  256x16x16 and 256x16x12, rate 8 behind the 96-bit header
                       encode3_aligned at 8 words per block (funnel-shifted
                       pairs, partials), four and three workgroups; 256x16x12
                       without the header too (the run-time full kernel at 8
                       words per block)
Fields: F1 as bench.py makes it, uniform noise (every block outruns its budget
into the slot's spare dwords, which the copy-out must leave behind) and F1 with
one spike.  The same stream object compressed twice gives the same bytes: every
launch zeroes its LDS slots.
"""
import ctypes

import numpy as np
import pytest

from pyoracle import params_rate

pytestmark = pytest.mark.gpu

# (nx, ny, nz), rate, dtype, header, byte offset of the stream in its buffer
CASES = {
    "one_group_rate16": ((64, 16, 16), 16, np.float32, False, 0),
    "row64_rate16": ((256, 16, 16), 16, np.float32, False, 0),
    "row64_rate12": ((256, 16, 16), 12, np.float32, False, 0),
    "row64_rate20": ((256, 16, 16), 20, np.float32, False, 0),
    "row64_rate16_f64": ((256, 16, 16), 16, np.float64, False, 0),
    "row64_rate16_start8": ((256, 16, 16), 16, np.float32, False, 8),
    "header_rate8": ((256, 16, 16), 8, np.float32, True, 0),
    "header_rate8_nz12": ((256, 16, 12), 8, np.float32, True, 0),
    "rate8_nz12": ((256, 16, 12), 8, np.float32, False, 0),
}
FIELDS = ["f1", "noise", "f1_spike"]
_cache = {}


def _field(kind, dims, dtype):
    """numpy (nz, ny, nx), made once per kind, shape and type and not modified."""
    key = (kind, dims, np.dtype(dtype).name)
    if key not in _cache:
        import torch
        import bench
        nx, ny, nz = dims
        if kind == "noise":
            a = np.random.default_rng(11).uniform(-1.0, 1.0, (nz, ny, nx)).astype(dtype)
        else:
            a = bench.smooth_slab_torch(torch, nx, ny, nz, 0, torch.device("cuda", 0)).cpu().numpy().astype(dtype)
            if kind == "f1_spike":
                a[nz // 2, 6, 133 % nx] *= 1000.0  # one value of one block
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def _dev_compress(product, a, dims, rate, header=False, start=0, repeat=1):
    """zfp_compress of a device copy of `a` into a device stream that begins
    `start` bytes into its buffer; the stream bytes of every call."""
    import torch
    lib = product.lib
    nx, ny, nz = dims
    ztype = 3 if a.dtype == np.float32 else 4
    d_field = torch.from_numpy(np.array(a)).cuda()
    field = lib.zfp_field_3d(ctypes.c_void_p(d_field.data_ptr()), ztype, nx, ny, nz)
    zs = lib.zfp_stream_open(None)
    lib.zfp_stream_set_rate(zs, float(rate), ztype, 3, 0)
    cap = lib.zfp_stream_maximum_size(zs, field) + 64
    d_out = torch.zeros(cap + start, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    bs = lib.stream_open(ctypes.c_void_p(d_out.data_ptr() + start), cap)
    lib.zfp_stream_set_bit_stream(zs, bs)
    outs = []
    for _ in range(repeat):
        lib.zfp_stream_rewind(zs)
        if header:
            assert lib.zfp_write_header(zs, field, 7) == 96
        n = lib.zfp_compress(zs, field)
        assert n > 0, lib.zfp_hip_last_error()
        outs.append(d_out[start:start + n].cpu().numpy().tobytes())
    lib.stream_close(bs)
    lib.zfp_stream_close(zs)
    lib.zfp_field_free(field)
    return outs


def _oracle_bytes(oracle, a, rate, bit_offset=0):
    ztype = 3 if a.dtype == np.float32 else 4
    words, end = oracle.compress_words(a, params_rate(rate, ztype, 3), bit_offset=bit_offset)
    return words.view(np.uint8).tobytes()[: (end + 63) // 64 * 8]


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("case", list(CASES))
def test_device_stream_matches_oracle(product, oracle, case, kind):
    dims, rate, dtype, header, start = CASES[case]
    a = _field(kind, dims, dtype)
    got, = _dev_compress(product, a, dims, rate, header=header, start=start)
    want = _oracle_bytes(oracle, a, rate, bit_offset=96 if header else 0)
    assert len(got) == len(want)
    skip = 12 if header else 0  # the header's bytes are the library's, not the codec's
    assert got[skip:] == want[skip:]


@pytest.mark.parametrize("kind", ["f1", "noise"])
@pytest.mark.parametrize("case", ["row64_rate16", "header_rate8"])
def test_same_stream_compressed_twice_gives_the_same_bytes(product, oracle, case, kind):
    dims, rate, dtype, header, start = CASES[case]
    a = _field(kind, dims, dtype)
    first, second = _dev_compress(product, a, dims, rate, header=header, start=start, repeat=2)
    want = _oracle_bytes(oracle, a, rate, bit_offset=96 if header else 0)
    skip = 12 if header else 0
    assert first[skip:] == second[skip:] == want[skip:]
