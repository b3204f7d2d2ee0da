"""The region row walker on the CPU: strided host rows <-> the packed image.

host_rows.h (region_rows, region_is_dense) is compiled with g++ into a
stand-alone program, with the address and undefined-behaviour sanitizers, and
run for every extent in {1, 2, 3, 5} per axis, 1D to 3D, element sizes 4 and 8,
through six host layouts (dense, padded y, x stride 2, negative y, negative z,
x stride 2 with negative y) in both directions: to the host every region element
holds the packed image's value and every other byte its sentinel, from the host
the packed image equals direct enumeration.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


def test_rows_both_directions_every_layout(tmp_path):
    exe = os.path.join(str(tmp_path), "rows_emu")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + HIP, "-o", exe, os.path.join(EMU, "rows_emu.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    # 2 element sizes x (4 + 16 + 64) extents x (6 layouts x 2 directions + the packed strides' dense test)
    assert "mismatches 0 of 2184" in r.stdout, r.stdout
