"""Registers of the flagship encode kernel (CPU test).

encode3_aligned_full<float, true, true, 16> runs four waves per SIMD: at most
128 vector registers and no scratch.  Read from its kernel descriptor in the
gfx950 code object of libzfp_hip.so, as tests/test_kernel_symbols.py reads the
scratch sizes: private_segment_fixed_size at byte 4, and the granulated VGPR
count in bits 0..5 of compute_pgm_rsrc1 at byte 48 (granules of 8 registers on
gfx950, accumulation registers included).
"""
import os
import struct

import pytest

from kdesc import MAGIC, _kernel_scratch, _sections
from test_kernel_symbols import LIB

KERNEL = "_ZN7zfp_amd20encode3_aligned_fullIfLb1ELb1ELi16EEEvPKT_NS_8GeometryENS_11CodecParamsEPmjjj"


def _descriptor(lib_bytes, kernel):
    """The 64-byte kernel descriptor of `kernel` from the gfx950 code objects."""
    secs = {nm: (off, size) for nm, _, off, size, _ in _sections(lib_bytes)}
    off, size = secs[".hip_fatbin"]
    fb = lib_bytes[off: off + size]
    i = 0
    while True:
        j = fb.find(MAGIC, i)
        if j < 0:
            return None
        n, = struct.unpack_from("<Q", fb, j + 24)
        p = j + 32
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", fb, p)
            p += 24
            triple = fb[p: p + tl].decode()
            p += tl
            if "gfx950" not in triple or not sz:
                continue
            elf = fb[j + o: j + o + sz]
            shoff, = struct.unpack_from("<Q", elf, 0x28)
            shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
            hdrs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + k * shentsize) for k in range(shnum)]
            for h in hdrs:
                if h[1] not in (2, 11):
                    continue
                stro = hdrs[h[6]][4]
                for k in range(h[5] // 24):
                    st_name, _, _, shndx, value, _ = struct.unpack_from("<IBBHQQ", elf, h[4] + k * 24)
                    if not st_name or shndx == 0 or shndx >= len(hdrs):
                        continue
                    nm = elf[stro + st_name: elf.index(b"\0", stro + st_name)].decode()
                    if nm == kernel + ".kd":
                        sec = hdrs[shndx]
                        kd = sec[4] + (value - sec[3])
                        return elf[kd: kd + 64]
        i = j + len(MAGIC)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libzfp_hip.so not built")
def test_rate16_encoder_fits_four_waves_without_scratch():
    kd = _descriptor(open(LIB, "rb").read(), KERNEL)
    assert kd is not None and len(kd) == 64, "kernel descriptor of the rate-16 encoder not found"
    scratch, = struct.unpack_from("<I", kd, 4)
    rsrc1, = struct.unpack_from("<I", kd, 48)
    vgprs = ((rsrc1 & 0x3f) + 1) * 8
    print("encode3_aligned_full<float, true, true, 16>: %d VGPRs (granule 8), %d bytes of scratch" % (vgprs, scratch))
    assert scratch == 0
    assert vgprs <= 128


@pytest.mark.skipif(not os.path.exists(LIB), reason="libzfp_hip.so not built")
def test_f64_aligned_full_scratch_is_what_it_was():
    """encode3_aligned_full<double, VEC> stands at its 168-VGPR bound and spills: 260 bytes per lane
    with 16-byte loads, 252 without.  The float kernels' opening (tables requested ahead of the
    block loads) is not theirs: holding the table quads across the loads cost them 20-32 bytes more."""
    sc = {k: v for k, v in _kernel_scratch(open(LIB, "rb").read()).items()
          if k.startswith("_ZN7zfp_amd20encode3_aligned_fullId")}
    assert len(sc) == 2, sorted(sc)
    for k, v in sc.items():
        assert v <= (260 if "IdLb1E" in k else 252), (k, v)
