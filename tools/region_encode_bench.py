"""Region-encode timing against the full encode (and decode) of the same field, same run.

  python tools/region_encode_bench.py [--n 1024] [--warmup 10] [--reps 20] [--out FILE]

A device-resident n^3 f32 stream of the bench.py smooth field (rate 16; rates 5
and 3.25 for the last two cases) and a device-resident source: the same field one plane
further along z, read in place with the field's strides.  Per case the region
call, the full zfp_hip_compress of the source field and the full
zfp_hip_decompress of the stream alternate, `warmup` untimed and `reps` timed
calls each; times are the kernel's, from HIP events through
zfp_hip_last_timing (median).  Cases (for n = 1024; they scale with n):
  (a) the whole field as a region        (d) [448:576]^3, aligned: no block is read
  (b) one z-slice [512:513, :, :]        (e) [450:575]^3: a read-modify-write shell
  (c) one x-slice [:, :, 512:513]        (f) (d) at rate 5 (320-bit blocks: 5 whole words)
                                         (g) (d) at rate 3.25 (208-bit blocks: the merge path)
Prints blocks written, region kernel ms, full-encode and full-decode kernel ms,
region / full encode, region / (full encode + full decode) -- what a caller
pays today to change the region -- and the region's time per block written.
Where every block of the region is covered (a, d, f, g) the written blocks are
checked against the full encode of the source field: (a) the whole stream bit
for bit, (d, f, g) through a region decode of both streams.
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
from pyoracle import params_rate  # noqa: E402


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
    lib.zfp_hip_compress_region.restype = i32
    lib.zfp_hip_compress_region.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, vp]
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
    source = smooth_slab_torch(torch, n, n, n, 1, dev)
    full_out = torch.empty_like(field)
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

    def encode(j, data, cap):
        words = torch.zeros(cap, dtype=torch.int64, device=dev)
        end = ctypes.c_uint64()
        if not lib.zfp_hip_compress(ctypes.byref(j), data.data_ptr(), words.data_ptr(), cap, 0, 0, -1, None,
                                    ctypes.byref(end)):
            fail()
        return words

    h, q = n // 2, n // 16
    cube = [(7 * q, 9 * q)] * 3
    odd = [(7 * q + 2, 9 * q - 1)] * 3
    whole = [(0, n)] * 3
    cases = [("a whole field", 16, whole, "stream"), ("b z-slice", 16, [(h, h + 1), (0, n), (0, n)], None),
             ("c x-slice", 16, [(0, n), (0, n), (h, h + 1)], None), ("d cube", 16, cube, "decode"),
             ("e cube with rmw shell", 16, odd, None), ("f cube rate 5", 5, cube, "decode"),
             ("g cube rate 3.25", 3.25, cube, "decode")]
    lines = ["region encode vs full encode (+ full decode), %d^3 f32, device stream and source, kernel ms "
             "(median of %d, %d warm-up)" % (n, a.reps, a.warmup),
             "%-24s %14s %10s %9s %9s %9s %12s %10s" % ("case", "blocks written", "region ms", "enc ms", "dec ms",
                                                       "/enc", "/(enc+dec)", "ns/block")]
    records = []
    streams = {}
    for name, rate, region, check in cases:  # region: numpy axis order
        params = params_rate(rate, 3, 3)
        j = job_of(params)
        cap = nblocks * params[1] // 64 + 4
        if rate not in streams:
            streams.clear()
            streams[rate] = encode(j, source, cap)
        words_src = streams[rate]  # the full encode of the source field
        words = encode(j, field, cap)  # every case starts from the field's own stream
        scratch = torch.zeros(cap, dtype=torch.int64, device=dev)
        lo = (ctypes.c_uint64 * 4)(*[r[0] for r in reversed(region)], 0)
        hi = (ctypes.c_uint64 * 4)(*[r[1] for r in reversed(region)], 0)
        ss = (ctypes.c_int64 * 4)(1, n, n * n, 0)
        src_ptr = source.data_ptr() + 4 * ((region[0][0] * n + region[1][0]) * n + region[2][0])
        blocks, end = ctypes.c_uint64(), ctypes.c_uint64()
        t_region, t_enc, t_dec = [], [], []
        for rep in range(a.warmup + a.reps):
            if not lib.zfp_hip_compress_region(ctypes.byref(j), lo, hi, src_ptr, ss, words.data_ptr(), cap, 0, -1,
                                               ctypes.byref(blocks)):
                fail()
            kr = kernel_ms(lib)
            if not lib.zfp_hip_compress(ctypes.byref(j), source.data_ptr(), scratch.data_ptr(), cap, 0, 0, -1, None,
                                        ctypes.byref(end)):
                fail()
            ke = kernel_ms(lib)
            if not lib.zfp_hip_decompress(ctypes.byref(j), full_out.data_ptr(), words.data_ptr(), cap, 0, -1, None,
                                          ctypes.byref(end)):
                fail()
            kd = kernel_ms(lib)
            if rep >= a.warmup:
                t_region.append(kr)
                t_enc.append(ke)
                t_dec.append(kd)
        same = None
        if check == "stream":
            same = bool(torch.equal(words, words_src))
        elif check == "decode":
            ext = [r[1] - r[0] for r in region]
            outs = []
            for w in (words, words_src):
                dst = torch.empty(ext, dtype=torch.float32, device=dev)
                ds = (ctypes.c_int64 * 4)(1, ext[2], ext[2] * ext[1], 0)
                if not lib.zfp_hip_decompress_region(ctypes.byref(j), lo, hi, dst.data_ptr(), ds, w.data_ptr(), cap, 0,
                                                     -1, None, None):
                    fail()
                outs.append(dst)
            same = bool(torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)))
        mr, me, md = statistics.median(t_region), statistics.median(t_enc), statistics.median(t_dec)
        rec = {"case": name, "n": n, "rate": rate, "blocks_written": blocks.value, "total_blocks": nblocks,
               "region_kernel_ms": mr, "full_encode_kernel_ms": me, "full_decode_kernel_ms": md,
               "ratio_to_encode": mr / me, "ratio_to_encode_plus_decode": mr / (me + md),
               "region_ns_per_block": 1e6 * mr / blocks.value, "full_encode_ns_per_block": 1e6 * me / nblocks,
               "region_ms_min_max": [min(t_region), max(t_region)], "full_encode_ms_min_max": [min(t_enc), max(t_enc)],
               "equals_full_encode": same}
        records.append(rec)
        lines.append("%-24s %14d %10.4f %9.4f %9.4f %9.4f %12.4f %10.3f%s" % (
            name, blocks.value, mr, me, md, mr / me, mr / (me + md), 1e6 * mr / blocks.value,
            "  DIFFERS FROM THE FULL ENCODE" if same is False else ""))
        del words, scratch
    lines.append("full encode: %.3f ns/block (case a's run)" % records[0]["full_encode_ns_per_block"])
    text = "\n".join(lines + [json.dumps(r) for r in records])
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(r["equals_full_encode"] is not False for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())
