"""The fixed-rate float32 encoder with class T (the planes of coefficients 0..3
from one table, three planes per write), scalar row bases and the pairwise cast:
whole streams byte for byte against the oracle, nothing excluded.

Field and stream are device resident and the stream start is aligned, so the
launcher takes encode3_aligned_full<float, true, true, SW> for every case: the
compile-time form at rate 16, the run-time-stride form at rate 8 and at rate 2
(two words per block, the fewest that kernel takes: a 128-bit budget, which ends
just after the class-T planes).
  256x16x4   256 blocks, one workgroup, a wave is one x-row (scalar row bases)
  512x8x8    two workgroups, two waves per x-row
  128x32x4   32 blocks per row: the per-lane position path, a wave spans two rows
Fields (F1 as bench.py makes it):
  f1          every wave smooth: the top planes class T
  const       one value everywhere: DC only, every plane of every group class T
  linear      a + bx + cy + dz: coefficients 0..3 only, class T down to the
              rounding noise
  f1_spikes   a spike 2^-j in one value of one block per wave, every j in 0..24
              with each of the lanes 0, 31 and 63 (lane 63 in the wave's second
              row on 128x32x4), over as many fields as that takes: one lane
              alone sets the wave's kT, on, above and below each group boundary
  noise       uniform [-1, 1): every wave wide (the coder without classes)
  zeros       all-zero blocks ("0" and padding)
  f1_special  one block with an inf, one with a NaN, one of denormals: the exact
              cast, which loads the block again through the same row bases
  f1_off16    F1 starting 16 bytes into its allocation
"""
import ctypes

import numpy as np
import pytest

from pyoracle import params_rate
from test_gpu_encode_plane_class import SHAPES, _f1, _wave_blocks

pytestmark = pytest.mark.gpu

FIELDS = ["f1", "const", "linear", "f1_spikes", "noise", "zeros", "f1_special", "f1_off16"]
RATES = [16, 8, 2]
_want = {}


def _fields(kind, dims):
    """The fields of a kind: numpy (nz, ny, nx) float32, one or a few."""
    nx, ny, nz = dims
    f1 = _f1(dims)
    if kind in ("f1", "f1_off16"):
        return [f1]
    if kind == "const":
        return [np.full((nz, ny, nx), np.float32(0.7314), np.float32)]
    if kind == "linear":
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        return [(0.25 + 0.001 * x - 0.013 * y + 0.05 * z).astype(np.float32)]
    if kind == "f1_spikes":
        # every j with each of the lanes 0, 31 and 63: 75 (j, lane) pairs dealt out
        # to the waves of as many fields as that takes.  The lane's block is block
        # first + lane of the raster order, so on 128x32x4 lane 63 lies in the
        # wave's second row.
        waves = _wave_blocks(dims)
        nbx, nby = nx // 4, ny // 4
        out = []
        for g in range(-(-75 // len(waves))):
            a = f1.copy()
            for w, (bx, by, bz) in enumerate(waves):
                c = (g * len(waves) + w) % 75
                j, lane = c % 25, (0, 31, 63)[c // 25]
                b = bx + nbx * (by + nby * bz) + lane
                lx, ly, lz = b % nbx, (b // nbx) % nby, b // (nbx * nby)
                a[4 * lz + 1, 4 * ly + 2, 4 * lx + 3] += np.float32(2.0 ** -j)
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


def _dev_compress(product, a, dims, rate, lead_bytes):
    import torch
    lib = product.lib
    nx, ny, nz = dims
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = torch.empty(flat.size + lead_bytes // 4, dtype=torch.float32, device="cuda")
    d_field = buf[lead_bytes // 4:]
    d_field.copy_(torch.from_numpy(np.array(flat)))
    assert d_field.data_ptr() == buf.data_ptr() + lead_bytes and d_field.data_ptr() % 16 == 0
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


def _oracle_stream(oracle, shape, kind, i, a, rate):
    """The oracle's stream, computed once per field and rate (f1_off16 is f1)."""
    key = (shape, "f1" if kind == "f1_off16" else kind, i, rate)
    if key not in _want:
        words, end = oracle.compress_words(a, params_rate(rate, 3, 3))
        _want[key] = words.view(np.uint8).tobytes()[: (end + 63) // 64 * 8]
    return _want[key]


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stream_matches_oracle(product, oracle, shape, kind, rate):
    dims = SHAPES[shape]
    for i, a in enumerate(_fields(kind, dims)):
        got = _dev_compress(product, a, dims, rate, 16 if kind == "f1_off16" else 0)
        want = _oracle_stream(oracle, shape, kind, i, a, rate)
        assert len(got) == len(want)
        if got != want:
            g, w = np.frombuffer(got, np.uint64), np.frombuffer(want, np.uint64)
            bad = np.flatnonzero(g != w)
            pytest.fail("field %d of %s: %d words differ, first in block %d" % (i, kind, bad.size, bad[0] // rate))
