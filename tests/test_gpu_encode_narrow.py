"""The float32 fixed-rate encoders' narrow high half, full-block gather and
per-wave block position, whole stream byte for byte against the oracle.

Field and stream are device resident (what bench.py times), so the launcher's
choice of kernel follows from the shape alone:
  256x16x16 rate 16   1,024 blocks in rows of 64: encode3_aligned_full without
                      partial blocks, a wave is one x-row (per-wave position)
  64x16x16 rate 16    256 blocks in rows of 16: the same kernel, a wave spans
                      four rows (per-lane position)
  256x16x16 rate 8    after a 96-bit header: encode3_aligned (unaligned start)
  256x16x18 rate 16   partial z blocks: the padded gather
Fields: F1 as bench.py makes it (every wave narrow), F1 with one value times
1,000 (that wave wide, the others narrow), uniform noise (every wave wide), F1
with one inf and one NaN (the exact-cast reload through the gather).  A wave
chooses its path on the device; the check is the stream.
"""
import ctypes

import numpy as np
import pytest

from pyoracle import params_rate

pytestmark = pytest.mark.gpu

# (nx, ny, nz), rate, header
SHAPES = {
    "row64": ((256, 16, 16), 16, False),
    "row16": ((64, 16, 16), 16, False),
    "header_rate8": ((256, 16, 16), 8, True),
    "partial_z": ((256, 16, 18), 16, False),
}
FIELDS = ["f1", "f1_spike", "noise", "f1_inf_nan"]
_cache = {}


def _field(kind, dims):
    """numpy (nz, ny, nx) float32, made once per kind and shape and not modified."""
    key = (kind, dims)
    if key not in _cache:
        import torch
        import bench
        nx, ny, nz = dims
        a = bench.smooth_slab_torch(torch, nx, ny, nz, 0, torch.device("cuda", 0)).cpu().numpy()
        if kind == "f1_spike":
            a[5, 6, 133 % nx] *= 1000.0  # one value of one block
        elif kind == "noise":
            a = np.random.default_rng(7).uniform(-1.0, 1.0, a.shape).astype(np.float32)
        elif kind == "f1_inf_nan":
            a[3, 9, 40] = np.inf
            a[nz - 1, 2, nx - 3] = np.nan
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def _dev_compress(product, d_field, dims, rate, header=False, strides=None, repeat=1):
    """zfp_compress of a device field into a device stream; the stream bytes of every call."""
    import torch
    lib = product.lib
    nx, ny, nz = dims
    field = lib.zfp_field_3d(ctypes.c_void_p(d_field.data_ptr()), 3, nx, ny, nz)
    if strides:
        lib.zfp_field_set_stride_3d(field, *strides)
    zs = lib.zfp_stream_open(None)
    lib.zfp_stream_set_rate(zs, float(rate), 3, 3, 0)
    cap = lib.zfp_stream_maximum_size(zs, field) + 64
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    bs = lib.stream_open(ctypes.c_void_p(d_out.data_ptr()), cap)
    lib.zfp_stream_set_bit_stream(zs, bs)
    outs = []
    for _ in range(repeat):
        lib.zfp_stream_rewind(zs)
        if header:
            assert lib.zfp_write_header(zs, field, 7) == 96
        n = lib.zfp_compress(zs, field)
        assert n > 0, lib.zfp_hip_last_error()
        outs.append(d_out[:n].cpu().numpy().tobytes())
    lib.stream_close(bs)
    lib.zfp_stream_close(zs)
    lib.zfp_field_free(field)
    return outs


def _oracle_bytes(oracle, a, rate, bit_offset=0):
    words, end = oracle.compress_words(a, params_rate(rate, 3, 3), bit_offset=bit_offset)
    return words.view(np.uint8).tobytes()[: (end + 63) // 64 * 8]


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_stream_matches_oracle(product, oracle, shape, kind):
    import torch
    dims, rate, header = SHAPES[shape]
    a = _field(kind, dims)
    got, = _dev_compress(product, torch.from_numpy(np.array(a)).cuda(), dims, rate, header=header)
    want = _oracle_bytes(oracle, a, rate, bit_offset=96 if header else 0)
    assert len(got) == len(want)
    skip = 12 if header else 0  # the header's bytes are the library's, not the codec's
    assert got[skip:] == want[skip:]


def test_strided_box_matches_oracle_on_the_same_box(product, oracle):
    """A 256x16x16 box inside a 260x20x20 allocation: row and plane strides
    that are not the extents, through the per-wave position."""
    import torch
    dims = (256, 16, 16)
    a = _field("f1_spike", dims)
    big = np.full((20, 20, 260), 7.5, dtype=np.float32)
    big[2:18, 2:18, 4:260] = a
    d_big = torch.from_numpy(big).cuda()
    d_box = d_big[2:18, 2:18, 4:260]
    got, = _dev_compress(product, d_box, dims, 16, strides=(1, 260, 260 * 20))
    assert got == _oracle_bytes(oracle, a, 16)


def test_timing_of_device_resident_compress_and_repeat(product, oracle):
    """zfp_hip_last_timing after a device-resident compress: a kernel time and a
    call time, the kernel's no longer than the call's; the same stream object
    used again gives the same bytes."""
    import torch
    dims = (256, 16, 16)
    a = _field("f1", dims)
    first, second = _dev_compress(product, torch.from_numpy(np.array(a)).cuda(), dims, 16, repeat=2)
    k, t = ctypes.c_double(), ctypes.c_double()
    assert product.lib.zfp_hip_last_timing(ctypes.byref(k), ctypes.byref(t)) == 1
    assert 0.0 < k.value <= t.value
    assert first == second == _oracle_bytes(oracle, a, 16)
