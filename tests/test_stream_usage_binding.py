"""ydc_usage_quanta / ydc_stream_usage_begin / _get / _find / _load without a GPU: the exported symbols, the
binding's structs against the header's layout, the host call against the model
(tests/stream_usage_model.py) through ctypes, the refusals that are decided before a device is touched,
and the arithmetic itself (yadcc_amd/csrc/usage_quanta.h) swept against its rule with 128-bit
intermediates by a stand-alone ASan + UBSan program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import stream_usage_model as U
from tests.conftest import ROOT
from yadcc_amd import binding, streaming

INVALID = -1  # YDC_ERR_INVALID_ARGUMENT
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def test_symbols_and_python_surface():
    for name in ("ydc_stream_usage_begin", "ydc_stream_usage_get", "ydc_stream_usage_find", "ydc_stream_usage_load",
                 "ydc_usage_quanta"):
        assert hasattr(binding.lib(), name), name
    for name in ("stream_usage_begin", "stream_usage_get", "stream_usage_find", "stream_usage_load"):
        assert callable(getattr(binding.Context, name)), name
    assert callable(binding.usage_quanta) and callable(streaming.usage)
    assert binding.lib().ydc_abi_version() == 8


def test_struct_layout():
    R, T = binding.UsageRow, binding.UsageTotals
    assert ctypes.sizeof(R) == 48
    assert [getattr(R, k).offset for k, _ in R._fields_] == [0, 4, 8, 16, 24, 32, 40]
    assert tuple(k for k, _ in R._fields_) == U.DTYPE.names == binding.USAGE_DTYPE.names
    assert binding.USAGE_DTYPE == U.DTYPE and binding.USAGE_DTYPE.itemsize == 48
    assert binding.USAGE_COLUMNS == U.COLUMNS
    assert [getattr(T, k).offset for k, _ in T._fields_] == [0, 8, 16, 24, 28] and ctypes.sizeof(T) == 32
    assert tuple(k for k, _ in T._fields_) == ("unattributed_time", "quanta", "ticks", "n_keys", "slots")


def test_the_host_call_is_the_model():
    edges = [I64_MIN, I64_MIN + 1, -1001, -1000, -999, -2, -1, 0, 1, 2, 999, 1000, 1001, I64_MAX - 1, I64_MAX]
    for q in (1, 2, 7, 1000, 1 << 40, I64_MAX):
        for a in edges:
            for b in edges:
                assert binding.usage_quanta(a, b, q) == U.quanta(a, b, q), (a, b, q)
    rng = np.random.default_rng(9)
    for _ in range(5000):
        a, b = (int(x) for x in rng.integers(I64_MIN, I64_MAX, 2, dtype=np.int64, endpoint=True))
        shift = int(rng.integers(0, 63))
        q = max(1, int(rng.integers(1, I64_MAX, dtype=np.int64)) >> shift)
        assert binding.usage_quanta(a, b, q) == U.quanta(a, b, q), (a, b, q)
        assert binding.usage_quanta(a >> shift, b >> shift, q) == U.quanta(a >> shift, b >> shift, q)
    assert binding.usage_quanta(49, 50, 50) == 1 and binding.usage_quanta(-50, -1, 50) == 0 and binding.usage_quanta(-1, 0, 50) == 1


def test_refusals_that_need_no_device():
    L = binding.lib()
    out = ctypes.c_uint64(77)
    for q in (0, -1, I64_MIN):
        assert L.ydc_usage_quanta(0, 10, q, ctypes.byref(out)) == INVALID and out.value == 77
        with pytest.raises(binding.YdcError):
            binding.usage_quanta(0, 10, q)
    assert L.ydc_usage_quanta(0, 10, 5, None) == INVALID
    # without a context: refused before anything is looked at
    n, rows = ctypes.c_uint32(77), np.full(2, 0xAB, binding.USAGE_DTYPE)
    tot = binding.UsageTotals(1, 2, 3, 4, 5)
    q = np.array([1, 2], np.uint32)
    for quantum in (1, 0, -5):
        assert L.ydc_stream_usage_begin(None, quantum, 0) == INVALID
    assert L.ydc_stream_usage_get(None, rows.ctypes.data, 2, ctypes.byref(n), ctypes.byref(tot), 0) == INVALID
    assert L.ydc_stream_usage_find(None, q.ctypes.data, 2, rows.ctypes.data) == INVALID
    assert L.ydc_stream_usage_load(None, rows.ctypes.data, 2, None) == INVALID
    assert n.value == 77 and (tot.unattributed_time, tot.quanta, tot.ticks, tot.n_keys, tot.slots) == (1, 2, 3, 4, 5)
    assert rows.tobytes() == np.full(2, 0xAB, binding.USAGE_DTYPE).tobytes()
    assert L.ydc_strerror(INVALID).decode() == "invalid argument"


def test_usage_quanta_header_under_sanitizers(tmp_path):
    """tests/native/usage_quanta_test.cc includes only usage_quanta.h; built the way `make usagequanta` builds
    it (a plain C++ compiler, ASan + UBSan) and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "usage_quanta_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "usage_quanta_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "USAGE-QUANTA-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
