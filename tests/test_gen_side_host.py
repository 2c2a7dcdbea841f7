"""The host side of a generated token's side outputs without a GPU: tests/host/gen_side_test.cpp -- umgen_amd/csrc/gen_side.h (GenSide::deliver, the
frame buffers' sizes, side_buffers) against element-by-element indexing, with sentinels around everything a delivery must leave alone -- compiled with
the host compiler and the flags of _lib.build_host_library, and run once."""
import os
import shutil
import subprocess

from umgen_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gen_side_header_against_elementwise_indexing(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++): the host library could not be built either"
    assert "gen_side.h" in _lib.HEADERS      # part of the library's source hash
    exe = str(tmp_path / "gen_side_test")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", _lib.CSRC, "-x", "c++",
                    os.path.join(ROOT, "tests", "host", "gen_side_test.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "gen_side_test: ok" in run.stdout, run.stdout[-4000:] + run.stderr[-2000:]
