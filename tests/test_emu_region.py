"""Region decode on the CPU: block mapping, clipped scatter, start table.

The mapping and scatter device functions of kernels_region.h are compiled with
g++ behind the stub runtime (tests/emu/stub) and run for every coded box with a
block-aligned origin and every region inside it, over fields of extents <= 9
(1D), <= (9, 6) (2D) and <= (9, 6, 5) (3D): every region element is written once
with the value of its own coordinates, nothing else is written, and the stream
blocks visited are exactly those that intersect the region.  The start-table
arithmetic is run with the wave scan's shuffle steps against a serial prefix sum
(per_wave 64 and 16; 1, 63, 64, 65 and 1000 blocks).
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


def test_region_mapping_scatter_and_start_table(tmp_path):
    exe = os.path.join(str(tmp_path), "region_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(EMU, "stub"), "-I" + HIP, "-o", exe,
                           os.path.join(EMU, "region_emu.cpp"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "region mismatches 0 of 5339078" in r.stdout, r.stdout
    assert "start table mismatches 0" in r.stdout, r.stdout
