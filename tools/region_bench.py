"""Region-decode timing against the full decode of the same stream, same run.

  python tools/region_bench.py [--n 1024] [--warmup 10] [--reps 20] [--out FILE]

A device-resident n^3 f32 stream of the bench.py smooth field (rate 16; and
precision 24 with its block index for the last case), a device-resident
destination.  Per case the region call and the full zfp_hip_decompress of the
same stream alternate, `warmup` untimed and `reps` timed calls each; times are
the kernel's, from HIP events through zfp_hip_last_timing (median).  Cases (for
n = 1024; they scale with n):
  (a) the whole field as a region        (d) [448:576]^3
  (b) one z-slice [512:513, :, :]        (e) [450:575]^3 (unaligned)
  (c) one x-slice [:, :, 512:513]        (f) (d) on a precision-24 stream with its index
Prints blocks read, region kernel ms, full-decode kernel ms, their ratio,
blocks_read / total blocks and the region's time per block read.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]

import torch  # noqa: E402  (one HIP runtime)
from bench import smooth_slab_torch  # noqa: E402
from pyoracle import params_precision, params_rate  # noqa: E402


class Job(ctypes.Structure):
    """zfp_hip_job (include/zfp_hip.h)."""
    _fields_ = [("type", ctypes.c_int32), ("dims", ctypes.c_int32), ("n", ctypes.c_uint64 * 4),
                ("s", ctypes.c_int64 * 4), ("f", ctypes.c_uint64 * 4), ("e", ctypes.c_uint64 * 4),
                ("minbits", ctypes.c_uint32), ("maxbits", ctypes.c_uint32), ("maxprec", ctypes.c_uint32),
                ("minexp", ctypes.c_int32)]


def bind(path):
    lib = ctypes.CDLL(path)
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    lib.zfp_hip_compress.restype = i32
    lib.zfp_hip_compress.argtypes = [vp, vp, vp, u64, u64, u64, i32, vp, vp]
    lib.zfp_hip_decompress.restype = i32
    lib.zfp_hip_decompress.argtypes = [vp, vp, vp, u64, u64, i32, vp, vp]
    lib.zfp_hip_decompress_region.restype = i32
    lib.zfp_hip_decompress_region.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, vp, vp]
    lib.zfp_hip_index_create.restype = vp
    lib.zfp_hip_index_free.argtypes = [vp]
    lib.zfp_hip_last_timing.restype = i32
    lib.zfp_hip_last_timing.argtypes = [vp, vp]
    lib.zfp_hip_last_error.restype = ctypes.c_char_p
    return lib


def kernel_ms(lib):
    k = ctypes.c_double()
    assert lib.zfp_hip_last_timing(ctypes.byref(k), None)
    return k.value


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
    full_out = torch.empty_like(field)
    nblocks = ((n + 3) // 4) ** 3

    def job_of(params):
        j = Job()
        j.type, j.dims = 3, 3
        for k in range(3):
            j.n[k], j.e[k] = n, n
        j.s[0], j.s[1], j.s[2] = 1, n, n * n
        j.minbits, j.maxbits, j.maxprec, j.minexp = params
        return j

    def encode(params, with_index):
        j = job_of(params)
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

    h, q = n // 2, n // 16
    cube = [(7 * q, 9 * q)] * 3
    odd = [(7 * q + 2, 9 * q - 1)] * 3
    whole = [(0, n)] * 3
    fixed = encode(params_rate(16, 3, 3), False)
    var = encode(params_precision(24), True)
    cases = [("a whole field", fixed, whole), ("b z-slice", fixed, [(h, h + 1), (0, n), (0, n)]),
             ("c x-slice", fixed, [(0, n), (0, n), (h, h + 1)]), ("d cube", fixed, cube),
             ("e cube unaligned", fixed, odd), ("f cube precision 24 + index", var, cube)]
    lines = ["region decode vs full decode, %d^3 f32, device stream and destination, kernel ms (median of %d, %d warm-up)"
             % (n, a.reps, a.warmup),
             "%-30s %12s %10s %10s %8s %10s %12s" % ("case", "blocks read", "region ms", "full ms", "ratio",
                                                      "blocks/all", "ns/block")]
    records = []
    for name, (j, words, cap, idx), region in cases:  # region: numpy axis order
        ext = [hi - lo for lo, hi in region]
        dst = torch.empty(ext, dtype=torch.float32, device=dev)
        lo = (ctypes.c_uint64 * 4)(*[r[0] for r in reversed(region)], 0)
        hi = (ctypes.c_uint64 * 4)(*[r[1] for r in reversed(region)], 0)
        ds = (ctypes.c_int64 * 4)(1, ext[2], ext[2] * ext[1], 0)
        blocks, end = ctypes.c_uint64(), ctypes.c_uint64()
        t_region, t_full = [], []
        for rep in range(a.warmup + a.reps):
            if not lib.zfp_hip_decompress_region(ctypes.byref(j), lo, hi, dst.data_ptr(), ds, words.data_ptr(), cap, 0,
                                                 -1, idx, ctypes.byref(blocks)):
                raise RuntimeError(lib.zfp_hip_last_error().decode())
            kr = kernel_ms(lib)
            if not lib.zfp_hip_decompress(ctypes.byref(j), full_out.data_ptr(), words.data_ptr(), cap, 0, -1, idx,
                                          ctypes.byref(end)):
                raise RuntimeError(lib.zfp_hip_last_error().decode())
            kf = kernel_ms(lib)
            if rep >= a.warmup:
                t_region.append(kr)
                t_full.append(kf)
        sl = tuple(slice(lo_, hi_) for lo_, hi_ in region)
        same = bool((dst.view(torch.int32) == full_out[sl].view(torch.int32)).all().item())
        mr, mf = statistics.median(t_region), statistics.median(t_full)
        rec = {"case": name, "n": n, "blocks_read": blocks.value, "total_blocks": nblocks, "region_kernel_ms": mr,
               "full_kernel_ms": mf, "ratio": mr / mf, "blocks_fraction": blocks.value / nblocks,
               "region_ns_per_block": 1e6 * mr / blocks.value, "full_ns_per_block": 1e6 * mf / nblocks,
               "region_ms_min_max": [min(t_region), max(t_region)], "full_ms_min_max": [min(t_full), max(t_full)],
               "equals_full_decode": same}
        records.append(rec)
        lines.append("%-30s %12d %10.4f %10.4f %8.4f %10.6f %12.3f%s" % (
            name, blocks.value, mr, mf, mr / mf, blocks.value / nblocks, 1e6 * mr / blocks.value,
            "" if same else "  DIFFERS FROM THE FULL DECODE"))
        del dst
    lines.append("full decode: %.3f ns/block (case a's run)" % records[0]["full_ns_per_block"])
    text = "\n".join(lines + [json.dumps(r) for r in records])
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for _, _, _, idx in (fixed, var):
        if idx:
            lib.zfp_hip_index_free(idx)
    return 0 if all(r["equals_full_decode"] for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())
