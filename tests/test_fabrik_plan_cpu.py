"""The host arithmetic of a FABRIK launch (csrc/ik_fabrik_plan.cpp) on the CPU:
tests/host/fabrik_plan_check.cpp, a stand-alone program built with
AddressSanitizer + UndefinedBehaviorSanitizer, checks tol_threshold by its
definition over every binade, the error band's properties, fabrik_qmax exactly and
the launch plan case by case (the program's header says how).
tests/test_band_cpu.py uses the same program (`--band`, `build_check`)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CLANGXX = "/opt/rocm/llvm/bin/clang++"  # csrc/Makefile HOSTCXX
CSRC = os.path.join(ROOT, "inversekinematicsann_amd", "csrc")
needs_clang = pytest.mark.skipif(not os.path.exists(CLANGXX),
                                 reason="the ROCm clang++ is not installed")


def build_check(tmp_dir):
    exe = os.path.join(str(tmp_dir), "fabrik_plan_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "fabrik_plan_check.cpp"),
                    os.path.join(CSRC, "ik_fabrik_plan.cpp"), "-o", exe], check=True)
    return exe


def run_check(exe, *args):
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


@needs_clang
def test_fabrik_plan_check(tmp_path):
    out = run_check(build_check(tmp_path))
    assert "fabrik_plan_check ok" in out, out[-4000:]
