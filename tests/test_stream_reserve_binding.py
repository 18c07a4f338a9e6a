"""ydc_stream_caps / ydc_stream_reserve without a GPU: the binding's struct has the header's layout,
the library exports the two entry points, and the Context has its two methods."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT
from yadcc_amd import binding

HEADER = os.path.join(ROOT, "include", "yadcc_dispatch.h")


def header_fields():
    """The fields of `typedef struct ydc_stream_caps { ... }` in declaration order."""
    src = open(HEADER).read()
    body = re.search(r"typedef struct ydc_stream_caps \{(.*?)\} ydc_stream_caps;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.fullmatch(r"\s*uint32_t\s+[a-z_,\s]+;\s*", body), body  # ten uint32_t, nothing else
    return re.findall(r"max_[a-z_]+", body)


def test_struct_layout_follows_the_header():
    names = [k for k, _ in binding.StreamCaps._fields_]
    assert names == header_fields() and len(names) == 10
    assert all(t is ctypes.c_uint32 for _, t in binding.StreamCaps._fields_)
    assert ctypes.sizeof(binding.StreamCaps) == 40
    assert [getattr(binding.StreamCaps, k).offset for k in names] == list(range(0, 40, 4))


def test_symbols_and_methods():
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "lib"], cwd=ROOT)
    lib = ctypes.CDLL(binding.LIB_PATH)
    for name in ("ydc_stream_caps_get", "ydc_stream_reserve"):
        assert name in binding.ABI_SYMBOLS and hasattr(lib, name), name
    assert binding.lib().ydc_stream_reserve.argtypes[1]._type_ is binding.StreamCaps
    assert callable(binding.Context.stream_caps) and callable(binding.Context.stream_reserve)
    # Neither call touches a device before it has looked at its arguments.
    assert lib.ydc_stream_reserve(None, None) == -1 and lib.ydc_stream_caps_get(None, None) == -1


def test_unknown_capacity_is_a_type_error():
    ctx = object.__new__(binding.Context)  # (no device: only the keyword check is reached)
    with pytest.raises(TypeError, match="max_lease"):
        binding.Context.stream_reserve(ctx, max_lease=5)
