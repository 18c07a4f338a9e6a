"""ydc_fair_level / ydc_stream_quota_fair / ydc_stream_quota_fair_result without a GPU: the host call
against the model (tests/stream_fair_model.py) through ctypes, the refusals that are decided before a
device is touched, the binding's struct against the header's layout, and the arithmetic itself
(yadcc_amd/csrc/fair_level.h) swept against the literal fill by a stand-alone ASan + UBSan program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import stream_fair_model as F
from tests.conftest import ROOT
from yadcc_amd import binding, streaming

UNL = F.UNLIMITED
INVALID = -1  # YDC_ERR_INVALID_ARGUMENT


def _level(askers, others, pool):
    h = [x[0] for x in askers]
    a = [x[1] for x in askers]
    caps = [UNL if x[2] is None else x[2] for x in askers]
    return binding.fair_level(h, a, caps, others=others, pool=pool)


def test_the_host_call_is_the_model():
    rng = np.random.default_rng(5)
    seen = set()
    for it in range(4000):
        large = it % 5 == 4
        top = (1 << 32) - 1 if large else 30
        askers = []
        for _ in range(int(rng.integers(0, 7))):
            h, a = int(rng.integers(0, top)), int(rng.integers(0, top))
            askers.append((h, a, int(rng.integers(0, top)) if rng.random() < 0.25 else None))  # (never UNL itself)
        others = int(rng.integers(0, 1 << 33 if large else 40))
        pool = int(rng.integers(0, 1 << 34 if large else 160))
        want = F.level(askers, others, pool)
        assert _level(askers, others, pool) == want, (askers, others, pool)
        seen.add("unl" if want == UNL else "zero" if want == 0 else "mid")
    assert seen == {"unl", "zero", "mid"}


def test_the_hand_vector_and_conventions():
    hand = [(0, 10, None), (3, 10, None), (8, 4, None)]
    assert _level(hand, 2, 20) == 5
    assert binding.fair_level([0, 3, 8], [10, 10, 4], None, others=2, pool=20) == 5  # fixed_cap NULL: everybody fair
    assert binding.fair_level([], [], None, others=9, pool=0) == UNL                 # n == 0
    assert _level([(1, 5, 3), (0, 9, 0)], 7, 0) == UNL                               # nobody fair
    assert _level([(0, (1 << 32) - 1, None)], 0, (1 << 64) - 1) == F.POOL_MAX        # the pool saturates at 2^32 - 2
    assert _level([(0, 5, None)], (1 << 64) - 1, (1 << 64) - 1) == 0                 # others alone above every pool


def test_refusals_that_need_no_device():
    L = binding.lib()
    out = ctypes.c_uint32(77)
    one = np.ones(1, np.uint32)
    assert L.ydc_fair_level(one.ctypes.data, one.ctypes.data, None, 1, 0, 0, None) == INVALID
    assert L.ydc_fair_level(None, one.ctypes.data, None, 1, 0, 0, ctypes.byref(out)) == INVALID
    assert L.ydc_fair_level(one.ctypes.data, None, None, 1, 0, 0, ctypes.byref(out)) == INVALID
    assert out.value == 77
    assert L.ydc_fair_level(None, None, None, 0, 0, 0, ctypes.byref(out)) == 0 and out.value == UNL
    # without a context: refused before anything is looked at
    for mode, pool in ((binding.FAIR_REGISTRY, 100), (binding.FAIR_FIXED, 5), (binding.FAIR_OFF, 0), (3, 1),
                       (binding.FAIR_REGISTRY, 0)):
        assert L.ydc_stream_quota_fair(None, mode, pool, 0) == INVALID
    res = binding.FairResult()
    assert L.ydc_stream_quota_fair_result(None, ctypes.byref(res)) == INVALID
    assert binding.lib().ydc_strerror(INVALID).decode() == "invalid argument"


def test_struct_layout_and_python_surface():
    R = binding.FairResult
    assert ctypes.sizeof(R) == 64
    assert [getattr(R, k).offset for k, _ in R._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 60]
    assert tuple(k for k, _ in R._fields_) == F.RESULT_FIELDS
    for name in ("ydc_stream_quota_fair", "ydc_stream_quota_fair_result", "ydc_fair_level"):
        assert hasattr(binding.lib(), name), name
    assert callable(binding.fair_level) and callable(streaming.fair_share)
    assert callable(binding.Context.stream_quota_fair) and callable(binding.Context.stream_quota_fair_result)


def test_fair_level_header_under_sanitizers(tmp_path):
    """tests/native/fair_level_test.cc includes only fair_level.h; built the way `make fairlevel` builds it
    (a plain C++ compiler, ASan + UBSan) and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fair_level_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "fair_level_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "FAIR-LEVEL-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
