"""Batched region encode against a loop of single-region calls over the same entries, same run.

  python tools/regions_encode_bench.py [--n 1024] [--warmup 10] [--reps 20] [--out FILE]

Two device-resident n^3 f32 streams of the bench.py smooth field (rate 16;
rate 3.25 for the last case), one for the batch and one for the loop, and a
device-resident source: the same field one plane further along z, read in
place with the field's strides.  Per case one zfp_hip_compress_regions call on
the first stream and the loop of zfp_hip_compress_region calls over the same
entries on the second alternate, `warmup` untimed and `reps` timed rounds
each.  Two times per round and side: the kernel time from HIP events through
zfp_hip_last_timing (the loop's is the sum over its calls) and the wall time
(host clock around the call or the whole loop; every call ends with its own
synchronize).  Medians are reported.  After every round the two streams must
be equal word for word.  Cases (for n = 1024; sizes scale with n):
  (a) one entry, the whole field
  (b) 64 block-aligned 32^3 crops on a 4 x 4 x 4 lattice of pitch 256
  (c) (b) shifted by (1, 2, 3): read-modify-write shells
  (d) 256 single elements in distinct blocks
  (e) 64 crops of 32^3 that are neighbours in x (two rows of 32: a row of the
      field holds 32), at rate 3.25: neighbouring entries share stream words on
      the merge path
Host-resident streams are not timed: they add the staging of one span of the
stream and its copy back to both sides.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]

import torch  # noqa: E402  (one HIP runtime)
from bench import smooth_slab_torch  # noqa: E402
from pyoracle import params_rate  # noqa: E402
from region_encode_bench import Job, kernel_ms  # noqa: E402
from region_encode_bench import bind as bind_single  # noqa: E402


class SrcRegion(ctypes.Structure):
    """zfp_hip_src_region (include/zfp_hip.h)."""
    _fields_ = [("lo", ctypes.c_uint64 * 4), ("hi", ctypes.c_uint64 * 4), ("src", ctypes.c_void_p),
                ("src_stride", ctypes.c_int64 * 4)]


def bind(path):
    lib = bind_single(path)
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    lib.zfp_hip_compress_regions.restype = i32
    lib.zfp_hip_compress_regions.argtypes = [vp, vp, u64, vp, u64, u64, i32, vp]
    return lib


def cases_for(n):
    """[(name, rate, entries)], entries in numpy axis order."""
    import numpy as np
    c, pitch = max(4, n // 32), n // 4
    lattice = [(pitch * z, pitch * y, pitch * x) for z in range(4) for y in range(4) for x in range(4)]
    crops = [[(k, k + c) for k in corner] for corner in lattice]
    shifted = [[(k + s, k + s + c) for k, s in zip(corner, (1, 2, 3))] for corner in lattice]
    rng = np.random.default_rng(256)
    nb = (n + 3) // 4
    points = []
    for b in rng.choice(nb ** 3, size=256, replace=False):
        bi = np.unravel_index(int(b), (nb, nb, nb))
        at = [min(4 * int(i) + int(rng.integers(0, 4)), n - 1) for i in bi]
        points.append([(v, v + 1) for v in at])
    y0 = 14 * c  # 448 for n = 1024
    row = [[(y0, y0 + c), (y0 + c * r, y0 + c * (r + 1)), (c * k, c * (k + 1))] for r in range(2)
           for k in range(n // c)][:64]
    return [("a whole field", 16, [[(0, n)] * 3]), ("b 64 aligned crops", 16, crops),
            ("c 64 shifted crops", 16, shifted), ("d 256 elements", 16, points),
            ("e 64 x-neighbours rate 3.25", 3.25, row)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", help="also write the table and one JSON line per case to this file")
    ap.add_argument("--lib", default=os.path.join(REPO, "zfp-par_amd", "lib", "libzfp_hip.so"))
    a = ap.parse_args()
    lib = bind(a.lib)
    n = a.n
    dev = torch.device("cuda:0")
    field = smooth_slab_torch(torch, n, n, n, 0, dev)
    source = smooth_slab_torch(torch, n, n, n, 1, dev)
    torch.cuda.synchronize()
    nblocks = ((n + 3) // 4) ** 3

    def fail():
        raise RuntimeError(lib.zfp_hip_last_error().decode())

    def job_of(params):
        j = Job()
        j.type, j.dims = 3, 3
        for k in range(3):
            j.n[k], j.e[k] = n, n
        j.s[0], j.s[1], j.s[2] = 1, n, n * n
        j.minbits, j.maxbits, j.maxprec, j.minexp = params
        return j

    lines = ["batched region encode vs a loop of single calls, %d^3 f32, device stream and sources, ms "
             "(median of %d, %d warm-up)" % (n, a.reps, a.warmup),
             "%-30s %8s %10s %10s %10s %8s %10s %10s %8s" % ("case", "entries", "blocks", "batch krn", "loop krn",
                                                              "ratio", "batch wall", "loop wall", "ratio")]
    records = []
    streams = {}
    for name, rate, entries in cases_for(n):
        params = params_rate(rate, 3, 3)
        j = job_of(params)
        cap = nblocks * params[1] // 64 + 4
        if rate not in streams:
            streams.clear()
            base = torch.zeros(cap, dtype=torch.int64, device=dev)
            end = ctypes.c_uint64()
            if not lib.zfp_hip_compress(ctypes.byref(j), field.data_ptr(), base.data_ptr(), cap, 0, 0, -1, None,
                                        ctypes.byref(end)):
                fail()
            streams[rate] = base
        words_b = streams[rate].clone()  # every case starts from the field's own stream
        words_l = streams[rate].clone()
        torch.cuda.synchronize()  # (the library's calls run on their own streams, unordered with torch's copies)
        table = (SrcRegion * len(entries))()
        singles = []
        ss = (ctypes.c_int64 * 4)(1, n, n * n, 0)
        for t, r in zip(table, entries):
            lo = (ctypes.c_uint64 * 4)(*[x[0] for x in reversed(r)], 0)
            hi = (ctypes.c_uint64 * 4)(*[x[1] for x in reversed(r)], 0)
            ptr = source.data_ptr() + 4 * ((r[0][0] * n + r[1][0]) * n + r[2][0])
            t.lo, t.hi, t.src, t.src_stride = lo, hi, ptr, ss
            singles.append((lo, hi, ptr))
        blocks_b, blocks_1 = ctypes.c_uint64(), ctypes.c_uint64()
        kb, kl, wb, wl = [], [], [], []
        same = True
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            if not lib.zfp_hip_compress_regions(ctypes.byref(j), table, len(entries), words_b.data_ptr(), cap, 0, -1,
                                                ctypes.byref(blocks_b)):
                fail()
            t1 = time.perf_counter()
            k_batch = kernel_ms(lib)
            k_loop, blocks_l = 0.0, 0
            t2 = time.perf_counter()
            for lo, hi, ptr in singles:
                if not lib.zfp_hip_compress_region(ctypes.byref(j), lo, hi, ptr, ss, words_l.data_ptr(), cap, 0, -1,
                                                   ctypes.byref(blocks_1)):
                    fail()
                k_loop += kernel_ms(lib)  # (read between calls: inside the loop's wall time, as a caller's own work)
                blocks_l += blocks_1.value
            t3 = time.perf_counter()
            same = same and blocks_b.value == blocks_l and bool(torch.equal(words_b, words_l))
            if rep >= a.warmup:
                kb.append(k_batch)
                kl.append(k_loop)
                wb.append(1e3 * (t1 - t0))
                wl.append(1e3 * (t3 - t2))
        med = statistics.median
        rec = {"case": name, "n": n, "rate": rate, "entries": len(entries), "blocks_written": blocks_b.value,
               "batch_kernel_ms": med(kb), "loop_kernel_ms": med(kl), "kernel_ratio": med(kb) / med(kl),
               "batch_wall_ms": med(wb), "loop_wall_ms": med(wl), "wall_ratio": med(wb) / med(wl),
               "batch_kernel_ms_min_max": [min(kb), max(kb)], "loop_kernel_ms_min_max": [min(kl), max(kl)],
               "batch_wall_ms_min_max": [min(wb), max(wb)], "loop_wall_ms_min_max": [min(wl), max(wl)],
               "equals_loop_every_round": same}
        records.append(rec)
        lines.append("%-30s %8d %10d %10.4f %10.4f %8.4f %10.4f %10.4f %8.4f%s" % (
            name, len(entries), blocks_b.value, med(kb), med(kl), med(kb) / med(kl), med(wb), med(wl),
            med(wb) / med(wl), "" if same else "  DIFFERS FROM THE LOOP"))
        del words_b, words_l
    r0 = records[0]
    lines.append("(a) single call kernel ms min-max %.4f-%.4f, batched %.4f-%.4f; wall %.4f-%.4f, batched %.4f-%.4f" % (
        *r0["loop_kernel_ms_min_max"], *r0["batch_kernel_ms_min_max"], *r0["loop_wall_ms_min_max"],
        *r0["batch_wall_ms_min_max"]))
    text = "\n".join(lines + [json.dumps(r) for r in records])
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(r["equals_loop_every_round"] for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())
