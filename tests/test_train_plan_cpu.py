"""The host arithmetic of the training calls (csrc/ik_train_plan.cpp) on the CPU:
tests/host/train_plan_check.cpp, a stand-alone program built with AddressSanitizer +
UndefinedBehaviorSanitizer, checks the state and data block layouts, the epoch's
steps and validation chunks, the losses, Adam's step size and the refusals (the
program's header says how)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CLANGXX = "/opt/rocm/llvm/bin/clang++"  # csrc/Makefile HOSTCXX
CSRC = os.path.join(ROOT, "inversekinematicsann_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="the ROCm clang++ is not installed")
def test_train_plan_check(tmp_path):
    exe = os.path.join(str(tmp_path), "train_plan_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "train_plan_check.cpp"),
                    os.path.join(CSRC, "ik_train_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "train_plan_check ok" in r.stdout, r.stdout[-4000:]
