"""ydc_depart_count / ydc_stream_depart_begin, _stage, _result without a GPU: the binding's struct has the
header's layout, the library exports the three entry points, and the Context's three methods refuse what
ctypes or numpy would silently wrap before any device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from yadcc_amd import binding, streaming

HEADER = os.path.join(ROOT, "include", "yadcc_dispatch.h")
NAMES = ("ydc_stream_depart_begin", "ydc_stream_depart_stage", "ydc_stream_depart_result")
FIELDS = ["requestor_ip", "leases", "zombies", "waiting", "waiting_rows"]


def header_fields():
    """The fields of `typedef struct ydc_depart_count { ... }` in declaration order."""
    src = open(HEADER).read()
    body = re.search(r"typedef struct ydc_depart_count \{(.*?)\} ydc_depart_count;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.fullmatch(r"(\s*uint32_t\s+[a-z_,\s]+;)+\s*", body), body  # five uint32_t, nothing else
    return re.findall(r"[a-z_]+", re.sub(r"uint32_t", "", body))


def test_struct_layout_follows_the_header():
    names = [k for k, _ in binding.DepartCount._fields_]
    assert names == header_fields() == FIELDS
    assert all(t is ctypes.c_uint32 for _, t in binding.DepartCount._fields_)
    assert ctypes.sizeof(binding.DepartCount) == 20
    assert [getattr(binding.DepartCount, k).offset for k in names] == [0, 4, 8, 12, 16]
    dt = binding.DEPART_DTYPE
    assert dt.itemsize == 20 and list(dt.names) == FIELDS and [dt.fields[k][1] for k in FIELDS] == [0, 4, 8, 12, 16]
    assert all(dt.fields[k][0] == np.dtype("<u4") for k in FIELDS)


def test_symbols_and_methods():
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "lib"], cwd=ROOT)
    lib = ctypes.CDLL(binding.LIB_PATH)
    for name in NAMES:
        assert name in binding.ABI_SYMBOLS and hasattr(lib, name), name
        assert callable(getattr(binding.Context, name[4:]))
    assert binding.lib().ydc_stream_depart_result.argtypes[1]._type_ is binding.DepartCount
    assert binding.ABI_VERSION == 8 and len(binding.StreamCaps._fields_) == 10  # (additive: neither moves)
    # None of the calls touches a device before it has looked at its arguments.
    n = ctypes.c_uint32(7)
    assert lib.ydc_stream_depart_begin(None, 4) == -1 and lib.ydc_stream_depart_stage(None, None, 0) == -1
    assert lib.ydc_stream_depart_result(None, None, 0, ctypes.byref(n), None, None) == -1 and n.value == 7
    assert callable(streaming.dismiss) and streaming.DEPART_COLUMNS == tuple(FIELDS)


def test_what_numpy_would_wrap_is_refused_before_the_call():
    ctx = object.__new__(binding.Context)  # (no device: only the argument checks are reached)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError, match="uint32"):
            binding.Context.stream_depart_begin(ctx, bad)
        with pytest.raises(ValueError, match="uint32"):
            binding.Context.stream_depart_stage(ctx, [1, bad])
    for bad in (1.5, "4", None, True):
        with pytest.raises(TypeError, match="max_depart"):
            binding.Context.stream_depart_begin(ctx, bad)
    for bad in ([1.0, 2.0], ["10.0.0.1"], [[1, 2], [3, 4]], 5):
        with pytest.raises(TypeError, match="requestor"):
            binding.Context.stream_depart_stage(ctx, bad)
    with pytest.raises(TypeError):
        binding.Context.stream_depart_begin(ctx, max_departs=4)
    with pytest.raises(TypeError):
        binding.Context.stream_depart_stage(ctx, requestor=[1])


def test_the_staged_column_is_what_the_caller_wrote():
    keys = binding._depart_keys(np.array([0xFFFFFFFF, 0, 7, 7], np.uint64))
    assert keys.dtype == np.uint32 and keys.flags["C_CONTIGUOUS"] and list(keys) == [0xFFFFFFFF, 0, 7, 7]
    assert list(binding._depart_keys(np.arange(10, dtype=np.int64)[::3])) == [0, 3, 6, 9]
    assert len(binding._depart_keys([])) == 0 and binding._depart_keys(()).dtype == np.uint32
