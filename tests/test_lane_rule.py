"""Which device lane a pipelined batch takes (yadcc_amd/csrc/lane_rule.h) without a GPU: the
stand-alone ASan + UBSan program tests/native/lane_rule_test.cc checks every row of the rule — nothing
outstanding, independent of a batch on either lane, and each single reason to stay on lane 0 (COMMIT
on either side, every pair of aliasing outputs, a batch that is not enqueued, a caller's stream, a
group, streaming, lanes off, lane 0 not settled) behind a batch on lane 0 and behind one on lane 1."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_lane_rule_row_by_row_under_sanitizers(tmp_path):
    """Includes only lane_rule.h; built the way the sanitizer programs of tests/native/Makefile are,
    and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "lane_rule_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "lane_rule_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "LANE-RULE-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
