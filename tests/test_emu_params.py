"""The device block codecs in host emulation over the parameter sweep
(tests/params.py): tests/emu/param_emu.cpp runs encode_block3 / decode_block3
(with the fixed-rate and the planes-32..63 coders where the launchers choose
them), encode_block_n / decode_block_n for 1D and 2D and the 4D quad codec
against the C oracle, for every rate, precision, tolerance and expert tuple,
over ladder blocks of every exponent.

The same program is built a second time with -fsanitize=address,undefined --
a stand-alone program, nothing preloaded -- with slots and staging buffers of
the launchers' sizes as exact heap blocks: an out-of-slot access at an untried
parameter shows here, on the CPU.
"""
import os
import subprocess

import pytest

import params as P
from test_param_sweep_oracle import AXES, codec_params, param_list, ztype_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(REPO, "tests", "emu")
HIP = os.path.join(REPO, "zfp-par_amd", "csrc", "hip")


def sweep_lines():
    lines, cases = [], 0
    for dtype in ("float32", "float64"):
        zt = ztype_of(dtype)
        lines.append("e %d %s" % (zt, " ".join(str(e) for e in P.ladder_exponents(dtype))))
        seen = set()
        todo = [(dims, codec_params(axis, param, dtype, dims)) for axis in AXES for dims in (1, 2, 3, 4)
                for param in param_list(axis, dtype)]
        for dims, cp in todo:
            if (dims, cp) not in seen:
                seen.add((dims, cp))
                lines.append("p %d %d %d %d %d %d" % ((zt, dims) + tuple(cp)))
                cases += 1
    return "\n".join(lines) + "\n", cases


@pytest.fixture(scope="module")
def emu_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("param_emu"))
    obj = os.path.join(d, "zfp_oracle.o")
    subprocess.check_call(["gcc", "-O2", "-c", "-I" + os.path.join(REPO, "oracle"), "-o", obj,
                           os.path.join(REPO, "oracle", "zfp_oracle.c")])
    return d, obj


def _build(d, obj, name, flags):
    exe = os.path.join(d, name)
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I" + os.path.join(EMU, "stub"), "-I" + HIP, "-o", exe,
                           os.path.join(EMU, "param_emu.cpp"), obj, "-pthread", "-lm"])
    return exe


def _run(exe, env=None):
    text, cases = sweep_lines()
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=3000, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) == cases and int(last[3]) > 200 * cases and int(last[5]) == 0, r.stdout
    return r


def test_device_codecs_match_oracle_over_the_sweep(emu_dir):
    d, obj = emu_dir
    _run(_build(d, obj, "param_emu", ["-O2"]))


def _sanitizer_missing(d):
    """Why -fsanitize=address,undefined cannot be used here, or None."""
    src = os.path.join(d, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", os.path.join(d, "probe"), src],
                       capture_output=True, text=True)
    if r.returncode != 0:
        return "g++ cannot link -fsanitize=address,undefined: " + r.stderr.strip().splitlines()[-1]
    r = subprocess.run([os.path.join(d, "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        return "a sanitized program does not start here: " + (r.stderr.strip().splitlines() or ["?"])[-1]
    return None


def test_device_codecs_over_the_sweep_clean_under_sanitizers(emu_dir):
    d, obj = emu_dir
    why = _sanitizer_missing(d)
    if why:
        pytest.skip(why)
    exe = _build(d, obj, "param_emu_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0"
    r = _run(exe, env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
