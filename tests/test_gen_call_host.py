"""The argument checks of the generation entry points without a GPU: tests/host/gen_call_test.cpp -- umgen_amd/csrc/gen_call.h (the call record every
rung of umgen_rollout* / umgen_frame* fills, and what check_gen_call refuses of it: codes, whole messages, order) -- compiled with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, and run once."""
import os
import shutil
import subprocess

from umgen_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gen_call_header_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++): the host library could not be built either"
    assert "gen_call.h" in _lib.HEADERS      # part of the library's source hash
    exe = str(tmp_path / "gen_call_test")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", _lib.CSRC, "-x", "c++", os.path.join(ROOT, "tests", "host", "gen_call_test.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "gen_call_test: ok" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
