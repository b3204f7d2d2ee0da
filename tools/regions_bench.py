"""Batched region decode against a loop of single-region calls over the same boxes, same run.

  python tools/regions_bench.py [--n 1024] [--warmup 10] [--reps 20] [--out FILE]

A device-resident n^3 f32 stream of the bench.py smooth field (rate 16; and
precision 24 with its block index for the last case), device-resident
destinations.  Per case one zfp_hip_decompress_regions call and the loop of
zfp_hip_decompress_region calls over the same boxes alternate, `warmup` untimed
and `reps` timed rounds each.  Two times per round and side: the kernel time
from HIP events through zfp_hip_last_timing (the loop's is the sum over its
calls) and the wall time of the batch (host clock around the call or the whole
loop; every call ends with its own synchronize).  Medians are reported.  Cases
(for n = 1024; the crop size scales with n):
  (a) one region, the whole field
  (b) 64 block-aligned 32^3 crops at seeded random positions
  (c) the same crops shifted by (1, 2, 3)
  (d) 256 single-element reads
  (e) case (b) on a precision-24 stream with its index
Every destination of the batch is compared with the loop's.
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
from pyoracle import params_precision, params_rate  # noqa: E402
from region_bench import Job, kernel_ms  # noqa: E402
from region_bench import bind as bind_single  # noqa: E402


class Region(ctypes.Structure):
    """zfp_hip_region (include/zfp_hip.h)."""
    _fields_ = [("lo", ctypes.c_uint64 * 4), ("hi", ctypes.c_uint64 * 4), ("dst", ctypes.c_void_p),
                ("dst_stride", ctypes.c_int64 * 4)]


def bind(path):
    lib = bind_single(path)
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    lib.zfp_hip_decompress_regions.restype = i32
    lib.zfp_hip_decompress_regions.argtypes = [vp, vp, u64, vp, u64, u64, i32, vp, vp]
    return lib


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
    nblocks = ((n + 3) // 4) ** 3

    def encode(params, with_index):
        j = Job()
        j.type, j.dims = 3, 3
        for k in range(3):
            j.n[k], j.e[k] = n, n
        j.s[0], j.s[1], j.s[2] = 1, n, n * n
        j.minbits, j.maxbits, j.maxprec, j.minexp = params
        bound = 9 + 63 + 64 * min(params[2], 32)
        per_block = max(min(bound, params[1]), params[0])
        cap = nblocks * per_block // 64 + 4
        words = torch.zeros(cap, dtype=torch.int64, device=dev)
        idx = lib.zfp_hip_index_create() if with_index else None
        end = ctypes.c_uint64()
        if not lib.zfp_hip_compress(ctypes.byref(j), field.data_ptr(), words.data_ptr(), cap, 0, 0, -1, idx,
                                    ctypes.byref(end)):
            raise RuntimeError(lib.zfp_hip_last_error().decode())
        return j, words, cap, idx

    import numpy as np
    rng = np.random.default_rng(64)
    c = max(4, n // 32)  # crop edge: 32 for n = 1024
    corners = [tuple(int(4 * v) for v in rng.integers(0, (n - c) // 4, size=3)) for _ in range(64)]
    crops = [[(k, k + c) for k in corner] for corner in corners]
    shifted = [[(k + s, k + s + c) for k, s in zip(corner, (1, 2, 3))] for corner in corners]
    points = [[(int(v), int(v) + 1) for v in rng.integers(0, n, size=3)] for _ in range(256)]
    fixed = encode(params_rate(16, 3, 3), False)
    var = encode(params_precision(24), True)
    del field
    cases = [("a whole field", fixed, [[(0, n)] * 3]), ("b 64 aligned crops", fixed, crops),
             ("c 64 shifted crops", fixed, shifted), ("d 256 elements", fixed, points),
             ("e 64 crops precision 24 + index", var, crops)]
    lines = ["batched region decode vs a loop of single calls, %d^3 f32, device stream and destinations, ms "
             "(median of %d, %d warm-up)" % (n, a.reps, a.warmup),
             "%-34s %8s %10s %10s %10s %8s %10s %10s %8s" % ("case", "regions", "blocks", "batch krn", "loop krn",
                                                              "ratio", "batch wall", "loop wall", "ratio")]
    records = []
    for name, (j, words, cap, idx), regions in cases:  # regions: numpy axis order
        exts = [[hi - lo for lo, hi in r] for r in regions]
        dst_b = [torch.zeros(e, dtype=torch.float32, device=dev) for e in exts]
        dst_l = [torch.zeros(e, dtype=torch.float32, device=dev) for e in exts]
        table = (Region * len(regions))()
        singles = []
        for t, r, e, db, dl in zip(table, regions, exts, dst_b, dst_l):
            lo = (ctypes.c_uint64 * 4)(*[x[0] for x in reversed(r)], 0)
            hi = (ctypes.c_uint64 * 4)(*[x[1] for x in reversed(r)], 0)
            ds = (ctypes.c_int64 * 4)(1, e[2], e[2] * e[1], 0)
            t.lo, t.hi, t.dst, t.dst_stride = lo, hi, db.data_ptr(), ds
            singles.append((lo, hi, dl.data_ptr(), ds))
        blocks_b, blocks_1 = ctypes.c_uint64(), ctypes.c_uint64()
        kb, kl, wb, wl = [], [], [], []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            if not lib.zfp_hip_decompress_regions(ctypes.byref(j), table, len(regions), words.data_ptr(), cap, 0, -1,
                                                  idx, ctypes.byref(blocks_b)):
                raise RuntimeError(lib.zfp_hip_last_error().decode())
            t1 = time.perf_counter()
            k_batch = kernel_ms(lib)
            k_loop, blocks_l = 0.0, 0
            t2 = time.perf_counter()
            for lo, hi, ptr, ds in singles:
                if not lib.zfp_hip_decompress_region(ctypes.byref(j), lo, hi, ptr, ds, words.data_ptr(), cap, 0, -1,
                                                     idx, ctypes.byref(blocks_1)):
                    raise RuntimeError(lib.zfp_hip_last_error().decode())
                k_loop += kernel_ms(lib)  # (read between calls: inside the loop's wall time, as a caller's own work)
                blocks_l += blocks_1.value
            t3 = time.perf_counter()
            if rep >= a.warmup:
                kb.append(k_batch)
                kl.append(k_loop)
                wb.append(1e3 * (t1 - t0))
                wl.append(1e3 * (t3 - t2))
        same = blocks_b.value == blocks_l and all(
            bool((x.view(torch.int32) == y.view(torch.int32)).all().item()) for x, y in zip(dst_b, dst_l))
        med = statistics.median
        rec = {"case": name, "n": n, "regions": len(regions), "blocks_read": blocks_b.value,
               "batch_kernel_ms": med(kb), "loop_kernel_ms": med(kl), "kernel_ratio": med(kb) / med(kl),
               "batch_wall_ms": med(wb), "loop_wall_ms": med(wl), "wall_ratio": med(wb) / med(wl),
               "batch_kernel_ms_min_max": [min(kb), max(kb)], "loop_kernel_ms_min_max": [min(kl), max(kl)],
               "batch_wall_ms_min_max": [min(wb), max(wb)], "loop_wall_ms_min_max": [min(wl), max(wl)],
               "equals_loop": same}
        records.append(rec)
        lines.append("%-34s %8d %10d %10.4f %10.4f %8.4f %10.4f %10.4f %8.4f%s" % (
            name, len(regions), blocks_b.value, med(kb), med(kl), med(kb) / med(kl), med(wb), med(wl),
            med(wb) / med(wl), "" if same else "  DIFFERS FROM THE LOOP"))
        del dst_b, dst_l
    r0 = records[0]
    lines.append("(a) single call kernel ms min-max %.4f-%.4f, batched %.4f-%.4f" % (
        *r0["loop_kernel_ms_min_max"], *r0["batch_kernel_ms_min_max"]))
    text = "\n".join(lines + [json.dumps(r) for r in records])
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for _, _, _, idx in (fixed, var):
        if idx:
            lib.zfp_hip_index_free(idx)
    return 0 if all(r["equals_loop"] for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())
