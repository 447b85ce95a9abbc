"""The ANN weight packing and model-buffer layout (csrc/ik_ann_pack.cpp) on the
CPU: tests/host/ann_pack_check.cpp, a stand-alone program built with
AddressSanitizer + UndefinedBehaviorSanitizer, checks every fragment order by its
inverse mapping into destinations of exactly the size functions' bytes, the split
planes' accuracy, and AnnLayout's rules (the program's header says how)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CLANGXX = "/opt/rocm/llvm/bin/clang++"  # csrc/Makefile HOSTCXX
CSRC = os.path.join(ROOT, "inversekinematicsann_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="the ROCm clang++ is not installed")
def test_ann_pack_check(tmp_path):
    exe = str(tmp_path / "ann_pack_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "ann_pack_check.cpp"),
                    os.path.join(CSRC, "ik_ann_pack.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ann_pack_check ok" in r.stdout, r.stdout[-4000:]
