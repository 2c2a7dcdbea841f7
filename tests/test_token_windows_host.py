"""Host token windows without a GPU: tests/host/token_windows_test.cpp -- umgen_amd/csrc/token_windows.h (the token view, gather_windows, frame_rows,
narrow_tokens, the window rule) against element-by-element indexing, and the rollout driver's window sequence against the slide / append sequence it
replaced -- compiled with the host compiler and the flags of _lib.build_host_library, and run once."""
import os
import shutil
import subprocess

from umgen_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_token_windows_header_against_elementwise_indexing(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++): the host library could not be built either"
    assert "token_windows.h" in _lib.HEADERS      # part of the library's source hash
    exe = str(tmp_path / "token_windows_test")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", _lib.CSRC, "-x", "c++",
                    os.path.join(ROOT, "tests", "host", "token_windows_test.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "token_windows_test: ok" in run.stdout, run.stdout[-4000:] + run.stderr[-2000:]
