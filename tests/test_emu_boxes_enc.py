"""Batched region encode on the CPU: the disjointness test and the merge through the batch's mapping.

host_disjoint.h (no HIP call) and the host-compilable parts of
kernels_boxes_enc.h are compiled with g++ behind the stub runtime
(tests/emu/stub).  The disjointness test is compared with the all-pairs brute
force on 3600 random sets of 1 to 40 boxes in 1D, 2D and 3D and on the edge
cases (touching at a face or a corner, sharing exactly one corner block,
identical, nested, 1000 coplanar one-block boxes with and without a duplicate),
swept along every axis: a reported pair is a true intersection, "none" means
none.  Then batches of two and three regions with disjoint block sets run
through box_wave, region_enc_pos and merge_word serially, at 208 bits per block
from bit 0 and from bit 96, waves in forward and reversed order, entries both
ways round: every bit of a touched block is written exactly once and by the
block that owns it, nothing else is written, and in most batches blocks of two
regions meet in one stream word.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


def test_disjointness_and_the_merge_of_a_batch(tmp_path):
    exe = os.path.join(str(tmp_path), "boxes_enc_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(EMU, "stub"), "-I" + HIP, "-o", exe,
                           os.path.join(EMU, "boxes_enc_emu.cpp"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "disjointness mismatches 0 of 3612 sets" in r.stdout, r.stdout
    assert "merge mismatches 0 of 40 batches, 36 with a word shared by two regions" in r.stdout, r.stdout
