"""Region encode on the CPU: the covered rule, the overlay and the merge.

The host-compilable part of kernels_region_enc.h is compiled with g++ behind
the stub runtime (tests/emu/stub) and run for every coded box with a
block-aligned origin and every region inside it, over fields of extents <= 9
(1D), <= (9, 6) (2D) and <= (9, 6, 5) (3D): `covered` equals direct
enumeration, and the overlay writes each region element exactly once with the
value of its own coordinates.  The copy-out's word and mask arithmetic is run
for every (maxbits in {9, 13, 32, 52, 64, 208, 320, 512}, bit0 in {0, 1, 32, 63,
96}) on a row of 70 blocks and every run of blocks, in two block orders: both
give the old words with exactly the run's bits replaced, and no word receives
both a plain store and a masked update.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


def test_region_encode_covered_overlay_and_merge(tmp_path):
    exe = os.path.join(str(tmp_path), "region_enc_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(EMU, "stub"), "-I" + HIP, "-o", exe,
                           os.path.join(EMU, "region_enc_emu.cpp"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "region mismatches 0 of 5339078" in r.stdout, r.stdout
    assert "merge mismatches 0 of 198800" in r.stdout, r.stdout  # 8 x 5 x 2485 runs x 2 orders
