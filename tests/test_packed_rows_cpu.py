"""Pack and unpack of the per-row index words of the row-per-lane kernels (csrc/packed_rows.h: the twenty-byte row-slot
words, the 16-bit column pairs of the coded fixed-width copy, the window rule) as plain C++: a stand-alone program built
with -fsanitize=address,undefined and run on the CPU."""

import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_pack_and_unpack_under_the_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "packed_rows"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "navier-stokes-solver_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "packed_rows_main.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("the sanitizer runtimes are not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "packed_rows ok" in run.stdout, run.stdout + run.stderr
