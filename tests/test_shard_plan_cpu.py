"""The arithmetic every rank of a sharded call must agree on
(csrc/ik_shard_plan.cpp) on the CPU: tests/host/shard_plan_check.cpp, a
stand-alone program built with AddressSanitizer + UndefinedBehaviorSanitizer,
checks the chunk plans and parts, the tail reduction, the histogram's bin edges
and its quantiles against brute force of its own (the program's header says how)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CLANGXX = "/opt/rocm/llvm/bin/clang++"  # csrc/Makefile HOSTCXX
CSRC = os.path.join(ROOT, "inversekinematicsann_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="the ROCm clang++ is not installed")
def test_shard_plan_check(tmp_path):
    exe = str(tmp_path / "shard_plan_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "shard_plan_check.cpp"),
                    os.path.join(CSRC, "ik_shard_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "shard_plan_check ok" in r.stdout, r.stdout[-4000:]
