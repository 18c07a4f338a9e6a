"""The arithmetic of a sharded batch (yadcc_amd/csrc/shard_plan.h) without a GPU: the stand-alone
ASan + UBSan program tests/native/shard_plan_test.cc checks the window's size, the pass groups, the
first pass without a change, the fallback's slicing and the `windowed` predicate against the rules
written out from their descriptions, on the named edges and on a seeded sweep."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_shard_plan_against_the_written_rules_under_sanitizers(tmp_path):
    """Includes only shard_plan.h; built the way the sanitizer programs of tests/native/Makefile are,
    and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "shard_plan_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "shard_plan_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SHARD-PLAN-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
