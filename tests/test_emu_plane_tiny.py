"""Host emulation of class T of the fixed-rate float32 coder: the planes of
coefficients 0..3 from one table, several planes per write (64 emulated lanes
per wave, CPU).

tests/emu/plane_tiny_emu.cpp, built like the programs of tests/test_emu.py: the
device headers behind the stub hip_runtime.h.
  The 80 entries of CoderTables::tiny against code_planes<32, false> run on one
  plane with n coefficients significant, for every (n, Pl).
  code_planes_fr32 with the threshold kT against code_planes<32, false>: kT at
  every value 0..32 (every position relative to the group boundaries), set by
  one lane alone; kT == kS; n reaching 4 in the first class-T plane; an
  all-zero block in the wave; thresholds raised by 1..3; budgets of 64, 128,
  256 and 1024 bits, the short ones ending inside or just after the class-T
  planes.
  The scan of planes_from_coeffs_auto: kT is the bit length of the OR over
  nb(c4..63), or larger.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


@pytest.fixture(scope="module")
def tiny_emu(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("emu_plane_tiny"))
    exe = os.path.join(d, "plane_tiny_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(EMU, "stub"), "-I" + HIP, "-o", exe,
                           os.path.join(EMU, "plane_tiny_emu.cpp"), "-lm"])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def _line(out, head):
    lines = [l for l in out.splitlines() if l.startswith(head)]
    assert len(lines) == 1, out
    return lines[0]


def test_table_entries_match_the_general_coder(tiny_emu):
    assert _line(tiny_emu.stdout, "table entries") == "table entries 80 mismatches 0", tiny_emu.stdout + tiny_emu.stderr


def test_crafted_thresholds_and_streams(tiny_emu):
    assert _line(tiny_emu.stdout, "crafted waves").endswith("mismatches 0"), tiny_emu.stdout + tiny_emu.stderr
    assert "do not cover" not in tiny_emu.stdout, tiny_emu.stdout


def test_scan_threshold_is_never_too_low(tiny_emu):
    assert "scan:" not in tiny_emu.stdout, tiny_emu.stdout
    assert _line(tiny_emu.stdout, "random waves").endswith("mismatches 0"), tiny_emu.stdout
    assert "do not reach" not in tiny_emu.stdout, tiny_emu.stdout


def test_plane_tiny_emulation_is_clean(tiny_emu):
    assert tiny_emu.returncode == 0, tiny_emu.stdout + tiny_emu.stderr
    assert tiny_emu.stdout.rstrip().endswith("mismatches 0"), tiny_emu.stdout
