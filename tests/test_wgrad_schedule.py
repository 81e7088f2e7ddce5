"""The backward's weight-gradient schedule (ssak_amd/csrc/wgrad_schedule.h) is host code without HIP: tests/wgrad_schedule_check.cpp
drives it with recording callables over layer counts up to the maximum, with and without a head, three tile shapes and
LayerDrop patterns (all kept, all dropped, alternating, one kept, seeded random), as an ordinary executable built with the
address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for cxx in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_wgrad_schedule_invariants_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or clang++) found")
    exe = tmp_path / "wgrad_schedule_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "wgrad_schedule_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cases ok" in run.stdout
