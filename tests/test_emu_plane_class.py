"""Host emulation of the fixed-rate float32 coder's plane classes (64 emulated
lanes per wave, CPU).

tests/emu/plane_class_emu.cpp, built like the programs of tests/test_emu.py: the
device headers behind the stub hip_runtime.h.  planes_from_coeffs_auto<P3, true>
returns the thresholds (ksw, kS) from the coefficients' widths, and
code_planes_fr32 with them must write the slot words of code_planes<32, false>:
  crafted waves with kS at every value 0..32 and ksw at every value -1..31, each
  set by one lane alone (lane 0, 31 or 63), thresholds exactly the targets;
  a lane with n' = 15 and xs = 0x7fff at n = 0 (31 bits in one write), plane 31
  zero and non-zero; thresholds raised by 1..3; budgets of 64, 128, 256 and
  1024 bits; and over 10^5 random waves, from smooth to dense, every plane
  classed S or M meets that body's preconditions in every lane.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


@pytest.fixture(scope="module")
def class_emu(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("emu_plane_class"))
    exe = os.path.join(d, "plane_class_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(EMU, "stub"), "-I" + HIP, "-o", exe,
                           os.path.join(EMU, "plane_class_emu.cpp"), "-lm"])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def _line(out, head):
    lines = [l for l in out.splitlines() if l.startswith(head)]
    assert len(lines) == 1, out
    return lines[0]


def test_crafted_thresholds_and_streams(class_emu):
    assert _line(class_emu.stdout, "crafted waves").endswith("mismatches 0"), class_emu.stdout + class_emu.stderr
    assert "do not cover" not in class_emu.stdout, class_emu.stdout


def test_full_fifteen_lane_is_one_write(class_emu):
    assert _line(class_emu.stdout, "full-15 lanes").endswith("mismatches 0"), class_emu.stdout + class_emu.stderr


def test_random_waves_meet_the_preconditions(class_emu):
    line = _line(class_emu.stdout, "random waves")
    assert line.startswith("random waves 100000 precondition violations 0 "), class_emu.stdout + class_emu.stderr
    assert line.endswith("mismatches 0"), class_emu.stdout


def test_budgets_cut_inside_class_s_planes(class_emu):
    line = _line(class_emu.stdout, "budget cuts inside a class-S plane:")
    cuts = [int(x) for x in line.split(":")[1].split("lanes")[0].split()]
    assert len(cuts) == 4 and min(cuts[:3]) >= 1000, line
    assert "do not cut" not in class_emu.stdout, class_emu.stdout


def test_plane_class_emulation_is_clean(class_emu):
    assert class_emu.returncode == 0, class_emu.stdout + class_emu.stderr
    assert class_emu.stdout.rstrip().endswith("mismatches 0"), class_emu.stdout
