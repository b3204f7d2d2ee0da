"""bench.py on the GPU at small --n: what a plain run does and leaves out, what
--full adds, and that --dump-outputs holds the stream of the timed zfp_compress
(checked against the CPU oracle's stream of the same field)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("decode_ms", "decode_kernel_ms", "decode_GBps", "decode_max_abs_err", "gather", "cpu_baseline",
             "bitexact_vs_reference")


def _bench(n, dump, extra=()):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--clock-warm-ms", "0", "--n", str(n), "--dump-outputs", str(dump)] + list(extra),
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    files = sorted(os.listdir(dump))
    assert files == ["stream.npy", "stream_nbytes.npy"]
    return d, np.load(os.path.join(dump, "stream.npy")), np.load(os.path.join(dump, "stream_nbytes.npy"))


def _oracle_stream(oracle, n):
    """The CPU oracle's rate-16 stream of bench.py's smooth n^3 field."""
    import torch
    import bench
    from pyoracle import params_rate
    a = bench.smooth_slab_torch(torch, n, n, n, 0, torch.device("cuda", 0)).cpu().numpy()
    words, end = oracle.compress_words(a, params_rate(16, 3, 3))
    return np.frombuffer(words.view(np.uint8).tobytes()[: (end + 63) // 64 * 8], dtype=np.uint8)


def test_plain_run_is_lean_and_dumps_a_stream_sample(tmp_path, oracle):
    # 176^3 at rate 16 is a 10.9 MB stream: above the 2^23 bytes stream.npy holds, so it is sampled
    import bench
    n = 176
    d, stream, nbytes = _bench(n, tmp_path / "out")
    for k in CONTRACT:
        assert k in d
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False and d["ms_per_step"] > 0
    assert d["calls"] == {"encode": 3, "decode": 0}
    for k in FULL_ONLY:
        assert k not in d
    want = _oracle_stream(oracle, n)
    assert nbytes.dtype == np.float64 and int(nbytes[0]) == d["config"]["stream_bytes_per_gpu"] == len(want)
    off = bench.stream_sample_offsets(len(want))
    assert off is not None and len(off) == bench.DUMP_STREAM_BYTES and off.max() < len(want)
    assert stream.dtype == np.float32 and np.array_equal(stream, want[off].astype(np.float32))


def test_full_run_adds_the_other_legs(tmp_path, oracle):
    n = 64
    d, stream, nbytes = _bench(n, tmp_path / "out", ["--full", "--no-cpu"])
    for k in CONTRACT:
        assert k in d
    assert d["full"] is True and d["calls"] == {"encode": 3, "decode": 3}
    # |v| < 1.5 and rate 16 leaves a 3D block about 13 bit planes: an error of 1e-2 would be a broken decode

    assert d["decode_ms"] > 0 and d["decode_GBps"] > 0 and d["decode_max_abs_err"] < 1e-2 and d["gather"] is None
    want = _oracle_stream(oracle, n)
    assert int(nbytes[0]) == len(want) == n ** 3 * 2
    assert stream.dtype == np.float32 and np.array_equal(stream, want.astype(np.float32))
