"""The host side of a sampling plan without a GPU: tests/host/sample_plan_test.cpp -- umgen_amd/csrc/sample_plan.h (the settings, index and table checks of
umgen_rollout_planned, the broadcast of a NULL bias_of, column f of the index) against element-by-element restatements -- compiled with the host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, and run once."""
import os
import shutil
import subprocess

from umgen_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_plan_header_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++): the host library could not be built either"
    assert "sample_plan.h" in _lib.HEADERS      # part of the library's source hash
    exe = str(tmp_path / "sample_plan_test")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", _lib.CSRC, "-x", "c++", os.path.join(ROOT, "tests", "host", "sample_plan_test.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "sample_plan_test: ok" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
