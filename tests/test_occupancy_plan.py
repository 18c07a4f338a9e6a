"""How much of a CU a batch asks for (yadcc_amd/csrc/occupancy_plan.h) without a GPU: the stand-alone
ASan + UBSan program tests/native/occupancy_plan_test.cc checks the width of a k_bin_sort workgroup
against a written table — narrow for a batch that may have a neighbour on the other lane, wide
otherwise, YDC_TUNE bin_threads=512|1024 wins, any other value is the rule's."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_occupancy_plan_row_by_row_under_sanitizers(tmp_path):
    """Includes only occupancy_plan.h; built the way the sanitizer programs of tests/native/Makefile
    are, and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "occupancy_plan_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "occupancy_plan_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OCCUPANCY-PLAN-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
