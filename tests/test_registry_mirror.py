"""The host mirror of the registry (yadcc_amd/csrc/registry_mirror.h) without a GPU: the stand-alone
ASan + UBSan program tests/native/registry_mirror_test.cc drives it and a naive model through seeded
sequences of uploads, heartbeat lists, removals and alias changes, and checks `structural` against
the rule written out from its description."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_mirror_against_a_naive_model_under_sanitizers(tmp_path):
    """Includes only the mirror's header; built the way the sanitizer programs of tests/native/Makefile
    are, and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "registry_mirror_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "registry_mirror_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "REGISTRY-MIRROR-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
