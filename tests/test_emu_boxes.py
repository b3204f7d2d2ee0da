"""Batched region decode on the CPU: the wave -> region mapping and the scatter through it.

The mapping of kernels_boxes.h (box_waves, box_wave) is compiled with g++ behind
the stub runtime (tests/emu/stub) and run for every ordering of one to four
regions with block counts from {1, 63, 64, 65, 128, 257} and for 1, 2, 64, 65
and 1000 one-block regions: the bisection equals a linear scan for every wave
number up to the first wave past the end, every (region, block) pair is visited
exactly once and no padding lane is active.  Then pairs and triples of regions
of fields of extents <= (9, 6, 5), overlapping ones included, are scattered
through the mapping into per-region guarded destinations: every region element
is written with its own coordinates, nothing else is written.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


def test_boxes_mapping_and_scatter(tmp_path):
    exe = os.path.join(str(tmp_path), "boxes_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(EMU, "stub"), "-I" + HIP, "-o", exe,
                           os.path.join(EMU, "boxes_emu.cpp"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mapping mismatches 0 of 1559 lists" in r.stdout, r.stdout
    assert "scatter mismatches 0 of 1728 region sets" in r.stdout, r.stdout
