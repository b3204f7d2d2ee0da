"""Host emulation of the float32 encoder's narrow high half (one lane, CPU).

tests/emu/narrow_emu.cpp, built like the programs of tests/test_emu.py: the
device headers behind the stub hip_runtime.h, in which a wave is one lane, so
the narrow or the full path is chosen per block.  Checked: the narrow plane
builder against the full one on all 64 plane words (random blocks with
coefficients 32..63 in [-170, 85], the edges 85 / -170 in single positions, an
all-zero high half), the exactness of the test (86 and -171 fail it), and
encode_block3_fixed on the narrow and on the full path against the oracle's
stream.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


@pytest.fixture(scope="module")
def narrow_emu(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("emu_narrow"))
    obj = os.path.join(d, "zfp_oracle.o")
    subprocess.check_call(["gcc", "-O2", "-c", "-I" + os.path.join(REPO, "oracle"), "-o", obj,
                           os.path.join(REPO, "oracle", "zfp_oracle.c")])
    exe = os.path.join(d, "narrow_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(EMU, "stub"), "-I" + HIP, "-o", exe,
                           os.path.join(EMU, "narrow_emu.cpp"), obj, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    return r


def test_narrow_builder_and_test_match_full_builder(narrow_emu):
    assert "builders mismatches 0" in narrow_emu.stdout, narrow_emu.stdout + narrow_emu.stderr


@pytest.mark.parametrize("rate", ["rate16", "rate8"])
def test_fixed_rate_block_matches_oracle_on_both_paths(narrow_emu, rate):
    lines = [l for l in narrow_emu.stdout.splitlines() if l.startswith(rate + ":")]
    assert lines and lines[0].endswith(" 0 bad"), narrow_emu.stdout + narrow_emu.stderr
    assert "do not cover both paths" not in narrow_emu.stdout, narrow_emu.stdout


def test_narrow_emulation_is_clean(narrow_emu):
    assert narrow_emu.returncode == 0, narrow_emu.stdout + narrow_emu.stderr
    assert narrow_emu.stdout.rstrip().endswith("mismatches 0"), narrow_emu.stdout
