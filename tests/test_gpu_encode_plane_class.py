"""The rate-16 float32 encoder with per-wave plane classes
(encode3_aligned_full<float, true, true, 16>: thresholds from the coefficients'
widths, one-write body for the top planes), whole stream byte for byte against
the oracle; and the same kernel's run-time-stride form at rate 8 (256x16x4),
which codes by the same classes.

Field and stream are device resident and the stream start is aligned, so the
launcher takes that kernel for every shape here:
  256x16x4   256 blocks, one workgroup, a wave is one x-row
  512x8x8    two workgroups, two waves per x-row
  128x32x4   32 blocks per row: the per-lane position path, a wave spans two rows
Fields (F1 as bench.py makes it):
  f1          every wave smooth: most planes class S
  f1_ramp     plus noise whose amplitude ramps 2^-28 .. 2^-2 along x, so the
              waves of a row differ in both thresholds, from narrow to wide
  f1_spikes   a spike 2^-j in one value of one block per wave, every j in 0..24
              over a few fields: one lane alone sets the wave's thresholds
  noise       uniform [-1, 1): every wave wide, every block outruns its budget
  zeros       all-zero blocks ("0" and padding)
  f1_special  one block with an inf, one with a NaN, one of denormals
"""
import ctypes

import numpy as np
import pytest

from pyoracle import params_rate

pytestmark = pytest.mark.gpu

SHAPES = {"one_group": (256, 16, 4), "two_groups": (512, 8, 8), "rows32": (128, 32, 4)}
FIELDS = ["f1", "f1_ramp", "f1_spikes", "noise", "zeros", "f1_special"]
_cache = {}


def _f1(dims):
    if dims not in _cache:
        import torch
        import bench
        nx, ny, nz = dims
        a = bench.smooth_slab_torch(torch, nx, ny, nz, 0, torch.device("cuda", 0)).cpu().numpy()
        a.setflags(write=False)
        _cache[dims] = a
    return _cache[dims]


def _wave_blocks(dims):
    """Block coordinates (bx, by, bz) of the first block of every wave."""
    nx, ny, nz = dims
    bxn, byn, bzn = nx // 4, ny // 4, nz // 4
    out = []
    for first in range(0, bxn * byn * bzn, 64):
        out.append((first % bxn, (first // bxn) % byn, first // (bxn * byn)))
    return out


def _fields(kind, dims):
    """The fields of a kind: numpy (nz, ny, nx) float32, one or a few."""
    nx, ny, nz = dims
    f1 = _f1(dims)
    if kind == "f1":
        return [f1]
    if kind == "f1_ramp":
        rng = np.random.default_rng(5)
        amp = np.exp2(-28.0 + 26.0 * np.arange(nx) / (nx - 1))
        return [(f1 + amp[None, None, :] * rng.uniform(-1.0, 1.0, f1.shape)).astype(np.float32)]
    if kind == "f1_spikes":
        waves = _wave_blocks(dims)
        out = []
        for g in range(-(-25 // len(waves))):
            a = f1.copy()
            for w, (bx, by, bz) in enumerate(waves):
                j = (g * len(waves) + w) % 25
                lane = (0, 31, 63)[(g + w) % 3] % (nx // 4)  # the block of the wave that holds the spike
                a[4 * bz + 1, 4 * by + 2, 4 * (bx + lane) + 3] += np.float32(2.0 ** -j)
            out.append(a)
        return out
    if kind == "noise":
        return [np.random.default_rng(11).uniform(-1.0, 1.0, (nz, ny, nx)).astype(np.float32)]
    if kind == "zeros":
        return [np.zeros((nz, ny, nx), np.float32)]
    assert kind == "f1_special"
    a = f1.copy()
    a[1, 1, 5] = np.inf
    a[2, 6, 4 * 17 + 2] = np.nan
    a[0:4, 4:8, 4 * 9:4 * 10] = np.float32(1e-45) * np.arange(64, dtype=np.float32).reshape(4, 4, 4)
    return [a]


def _dev_compress(product, a, dims, rate):
    import torch
    lib = product.lib
    nx, ny, nz = dims
    d_field = torch.from_numpy(np.array(a)).cuda()
    field = lib.zfp_field_3d(ctypes.c_void_p(d_field.data_ptr()), 3, nx, ny, nz)
    zs = lib.zfp_stream_open(None)
    lib.zfp_stream_set_rate(zs, float(rate), 3, 3, 0)
    cap = lib.zfp_stream_maximum_size(zs, field) + 64
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    bs = lib.stream_open(ctypes.c_void_p(d_out.data_ptr()), cap)
    lib.zfp_stream_set_bit_stream(zs, bs)
    n = lib.zfp_compress(zs, field)
    assert n > 0, lib.zfp_hip_last_error()
    got = d_out[:n].cpu().numpy().tobytes()
    lib.stream_close(bs)
    lib.zfp_stream_close(zs)
    lib.zfp_field_free(field)
    return got


def _check(product, oracle, shape, kind, rate):
    dims = SHAPES[shape]
    for i, a in enumerate(_fields(kind, dims)):
        got = _dev_compress(product, a, dims, rate)
        words, end = oracle.compress_words(a, params_rate(rate, 3, 3))
        want = words.view(np.uint8).tobytes()[: (end + 63) // 64 * 8]
        assert len(got) == len(want)
        if got != want:
            g, w = np.frombuffer(got, np.uint64), np.frombuffer(want, np.uint64)
            bad = np.flatnonzero(g != w)
            pytest.fail("field %d of %s: %d words differ, first in block %d" % (i, kind, bad.size, bad[0] // rate))


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rate16_stream_matches_oracle(product, oracle, shape, kind):
    _check(product, oracle, shape, kind, 16)


@pytest.mark.parametrize("kind", FIELDS)
def test_rate8_stream_matches_oracle(product, oracle, kind):
    """The run-time-stride form of the kernel (8 words per block, a 512-bit budget) codes by the same classes."""
    _check(product, oracle, "one_group", kind, 8)
