"""Host emulation of the fixed-rate float32 coder on a narrow wave's planes and
on its first plane (one lane, CPU).

tests/emu/fr32_flag_emu.cpp, built like the programs of tests/test_emu.py: the
device headers behind the stub hip_runtime.h.  code_planes_fr32, on planes
whose high half is zero from plane 8 up and on planes with something there,
must write the slot words of code_planes<32, false>.  The program also checks
that its plane sets cover n reaching 32 inside planes 31..8 and plane 31 zero
(no verbatim write is issued for it) and non-zero.  The wave-uniform narrow
flag these files were named for measured slower and was not kept;
the coder is called with its seven arguments.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


@pytest.fixture(scope="module")
def flag_emu(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("emu_fr32_flag"))
    exe = os.path.join(d, "fr32_flag_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(EMU, "stub"), "-I" + HIP, "-o", exe,
                           os.path.join(EMU, "fr32_flag_emu.cpp"), "-lm"])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def test_coder_on_narrow_planes_matches_code_planes(flag_emu):
    lines = [l for l in flag_emu.stdout.splitlines() if l.startswith("narrow planes mismatches")]
    assert len(lines) == 2 and all(l.startswith("narrow planes mismatches 0 ") for l in lines), \
        flag_emu.stdout + flag_emu.stderr
    assert "do not cover" not in flag_emu.stdout, flag_emu.stdout


def test_coder_on_wide_planes_matches_code_planes(flag_emu):
    lines = [l for l in flag_emu.stdout.splitlines() if l.startswith("wide planes mismatches")]
    assert len(lines) == 2 and all(l.endswith(" 0") for l in lines), flag_emu.stdout + flag_emu.stderr


def test_flag_emulation_is_clean(flag_emu):
    assert flag_emu.returncode == 0, flag_emu.stdout + flag_emu.stderr
    assert flag_emu.stdout.rstrip().endswith("mismatches 0"), flag_emu.stdout
