"""The staging block of the host-pointer batch calls, checked without a GPU: tests/host/staging_layout_check.cpp includes only
restartsqp_amd/csrc/rsqp_batch_staging.h (plain C++17), lays out the eight calls' blocks for a handful of shapes and takes each
through a round trip between heap blocks of exactly the computed size. Built here with the system's C++ compiler under
AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(_ROOT, "tests", "host", "staging_layout_check.cpp")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_staging_layout_under_sanitizers(tmp_path):
    cxx = _compiler()
    assert cxx, "no C++ compiler found (g++, c++, clang++)"
    exe = str(tmp_path / "staging_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", _SRC, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks held" in run.stdout
