"""Every kernel the host code can launch has gfx950 device code (CPU test).

A template kernel whose host launch stub is compiled but whose device code is
not instantiated makes HIP abort the calling process at launch ("could not
find the symbol"), breaking the C API's "return 0, stream untouched" contract.
This test reads libzfp_hip.so without a GPU: the host stubs from its symbol
table, the device kernels from the gfx950 code objects in its .hip_fatbin
section (clang offload bundles of ELF code objects), and checks that every stub
has a kernel descriptor (`<name>.kd`) in some code object.
"""
import os
import re
import subprocess

import pytest

from kdesc import _device_kernels, _kernel_scratch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "zfp-par_amd", "lib", "libzfp_hip.so")

_STUB = re.compile(r"^(_Z(?:N7zfp_amd)?L?)(\d+)__device_stub__(.*)$")


def _host_stub_kernels():
    out = subprocess.run(["nm", LIB], capture_output=True, text=True, check=True).stdout
    kernels = set()
    for line in out.splitlines():
        name = line.split()[-1]
        m = _STUB.match(name)
        if not m:
            continue
        n = int(m.group(2)) - len("__device_stub__")
        rest = m.group(3)
        kernels.add("%s%d%s" % (m.group(1), n, rest))
    return kernels


@pytest.mark.skipif(not os.path.exists(LIB), reason="libzfp_hip.so not built")
def test_every_host_kernel_stub_has_gfx950_code():
    data = open(LIB, "rb").read()
    device, objects = _device_kernels(data)
    host = _host_stub_kernels()
    assert objects >= 1, "no gfx950 code object in .hip_fatbin"
    assert len(host) > 20, "host kernel stubs not found (%d)" % len(host)
    missing = sorted(host - device)
    assert not missing, "kernels launched by the host without device code:\n  " + "\n  ".join(missing[:20])


@pytest.mark.skipif(not os.path.exists(LIB), reason="libzfp_hip.so not built")
def test_hot_kernels_use_no_scratch():
    """The float kernels (C2/C4/C5 paths) and the f64 decoders without short
    slots keep their plane registers in VGPRs: no private (scratch) segment.
    Scratch here means an unrolled plane loop fell back to memory (it did once:
    LLVM's pragma-unroll threshold), which costs HBM traffic on every launch.
    Exception: the float decode4 is compiled for 4 waves per SIMD (128 VGPRs,
    kernels4.h kDec4Waves) and spills a few scalars (<= 40 bytes per lane, no
    plane registers; 28 in round 6, 40 before its block state was parked in
    LDS), measured 20 % faster than 3 waves without spills.  The C3 kernels
    (f64, planes 32..63 only, 3 waves per SIMD at their 168-VGPR bound) are
    held to what round 6 left them: the encoder 32 bytes (48 when its
    wave-uniform values sat in VGPRs, written once per lane on the hot path),
    the short-slot decoder 60."""
    sc = _kernel_scratch(open(LIB, "rb").read())
    assert len(sc) > 20
    hot = {k: v for k, v in sc.items()
           if re.match(r"_ZN7zfp_amd(15encode3_(aligned|general)|20encode3_aligned_full|7decode3|7encode4|7decode4)If", k)}
    assert len(hot) >= 8, sorted(sc)[:10]
    bounded = {k: v for k, v in hot.items() if k.startswith("_ZN7zfp_amd7decode4If")}
    assert bounded and all(v <= 40 for v in bounded.values()), bounded
    assert all(v == 0 for k, v in hot.items() if k not in bounded), {k: v for k, v in hot.items() if v and k not in bounded}
    # f64 decoders without short slots: P[32] must stay in registers
    dnon = {k: v for k, v in sc.items() if k.startswith("_ZN7zfp_amd7decode3Id") and k.endswith("Lb0EEEvPT_NS_8GeometryENS_11CodecParamsENS_10DecodeArgsE")}
    assert dnon and all(v == 0 for v in dnon.values()), dnon
    # the C3 kernels: encode3_general<double, VEC, lossy, HI> and the short-slot decoder
    c3e = {k: v for k, v in sc.items() if re.match(r"_ZN7zfp_amd15encode3_generalIdLb[01]ELb0ELb1ELi3E", k)}
    c3d = {k: v for k, v in sc.items() if re.match(r"_ZN7zfp_amd7decode3IdLb[01]ELb0ELb1ELi3ELb1E", k)}
    assert c3e and all(v <= 32 for v in c3e.values()), c3e
    assert c3d and all(v <= 60 for v in c3d.values()), c3d
