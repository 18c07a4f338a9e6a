"""ydc_lease_filter / ydc_stream_inspect_select / ydc_stream_inspect_count without a GPU: the binding's
struct has the header's layout (48 bytes, every offset), the library exports the two entry points and
refuses a call without a context before it touches a device, the wrappers refuse what ctypes would
silently wrap, and the predicate itself (yadcc_amd/csrc/lease_filter.h) is swept against a second
restatement by a stand-alone ASan + UBSan program."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.conftest import ROOT
from yadcc_amd import binding, streaming

HEADER = os.path.join(ROOT, "include", "yadcc_dispatch.h")
NAMES = ("ydc_stream_inspect_select", "ydc_stream_inspect_count")
C_TYPES = {"uint32_t": (ctypes.c_uint32, 4), "uint8_t": (ctypes.c_uint8, 1), "int64_t": (ctypes.c_int64, 8),
           "uint64_t": (ctypes.c_uint64, 8)}


def header_layout():
    """(name, ctype, array length or None, offset) of every member of `typedef struct ydc_lease_filter`,
    laid out by C's rule (each member aligned to its own size), and the struct's size."""
    src = open(HEADER).read()
    body = re.search(r"typedef struct ydc_lease_filter \{(.*?)\} ydc_lease_filter;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out, off, widest = [], 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        t, size = C_TYPES[ctype]
        widest = max(widest, size)
        for name in (x.strip() for x in names.split(",")):
            m = re.fullmatch(r"([a-z_]+)(?:\[(\d+)\])?", name)
            count = int(m.group(2)) if m.group(2) else None
            off = (off + size - 1) // size * size
            out.append((m.group(1), t, count, off))
            off += size * (count or 1)
    return out, (off + widest - 1) // widest * widest


def test_struct_layout_follows_the_header():
    members, size = header_layout()
    assert size == 48 == ctypes.sizeof(binding.LeaseFilter)
    assert [m[0] for m in members] == [k for k, _ in binding.LeaseFilter._fields_] == [
        "fields", "servant_idx", "env_id", "requestor_ip", "zombie", "prefetch", "pad", "expires_before", "started_before",
        "after_id"]
    assert [m[3] for m in members] == [0, 4, 8, 12, 16, 17, 18, 24, 32, 40]
    for (name, t, count, off), (_, bt) in zip(members, binding.LeaseFilter._fields_):
        assert getattr(binding.LeaseFilter, name).offset == off, name
        assert bt is (t * count if count else t) or (count and bt._type_ is t and bt._length_ == count), name


def test_the_bits_follow_the_header():
    src = open(HEADER).read()
    bits = {k: int(v, 16) for k, v in re.findall(r"#define YDC_SEL_([A-Z_]+)\s+(0x[0-9a-fA-F]+)u", src)}
    assert bits == {"SERVANT": 1, "ZOMBIE": 2, "EXPIRES_BEFORE": 4, "AFTER_ID": 8, "ENV": 16, "REQUESTOR": 32,
                    "PREFETCH": 64, "STARTED_BEFORE": 128, "UNATTRIBUTED": 256}
    for k, v in bits.items():
        assert getattr(binding, "SEL_" + k) == v, k
    assert int(re.search(r"#define YDC_SELECT_MAX_FILTERS\s+(\d+)u", src).group(1)) == binding.SELECT_MAX_FILTERS == 64
    assert re.search(r"#define YDC_ABI_VERSION 8u", src) and binding.ABI_VERSION == 8


def test_symbols_and_methods():
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "lib"], cwd=ROOT)
    lib = ctypes.CDLL(binding.LIB_PATH)
    for name in NAMES:
        assert name in binding.ABI_SYMBOLS and hasattr(lib, name), name
        assert callable(getattr(binding.Context, name[4:]))
    L = binding.lib()
    assert L.ydc_stream_inspect_select.argtypes[1]._type_ is binding.LeaseFilter and len(L.ydc_stream_inspect_select.argtypes) == 13
    assert L.ydc_stream_inspect_count.argtypes[1]._type_ is binding.LeaseFilter
    assert callable(streaming.iter_tasks)
    # Neither call touches a device, or its outputs, before it has a context.
    f = binding.LeaseFilter()
    n, m = ctypes.c_uint32(7), ctypes.c_uint32(9)
    assert L.ydc_stream_inspect_select(None, ctypes.byref(f), *([None] * 8), 4, ctypes.byref(n), ctypes.byref(m)) == -1
    assert L.ydc_stream_inspect_count(None, ctypes.byref(f), 1, ctypes.addressof(m)) == -1
    assert (n.value, m.value) == (7, 9)


def test_the_filter_from_keywords():
    f = binding.lease_filter()
    assert f.fields == 0 and bytes(f) == bytes(48)
    f = binding.lease_filter(servant=3, zombie=1, expires_before=-5, after_id=(1 << 64) - 1, env_id=0, requestor_ip=0xFFFFFFFF,
                             prefetch=0, started_before=-(1 << 63), unattributed=True)
    assert f.fields == 0x1FF
    assert (f.servant_idx, f.zombie, f.expires_before, f.after_id) == (3, 1, -5, (1 << 64) - 1)
    assert (f.env_id, f.requestor_ip, f.prefetch, f.started_before) == (0, 0xFFFFFFFF, 0, -(1 << 63))
    assert binding.lease_filter(env_id=0).fields == binding.SEL_ENV  # (0 is a key, not "left out")
    assert binding.lease_filter(zombie=2).zombie == 2  # (the library refuses it, with its message)
    assert binding.lease_filter(unattributed=False).fields == 0


def test_what_ctypes_would_wrap_is_refused_before_the_call():
    for bad in ({"servant": -1}, {"servant": 1 << 32}, {"env_id": 1 << 32}, {"requestor_ip": -1}, {"after_id": -1},
                {"after_id": 1 << 64}, {"expires_before": 1 << 63}, {"started_before": -(1 << 63) - 1}, {"zombie": 256},
                {"prefetch": -1}):
        with pytest.raises(ValueError, match="does not fit"):
            binding.lease_filter(**bad)
    with pytest.raises(TypeError):
        binding.lease_filter(requestor=1)
    ctx = object.__new__(binding.Context)  # (no device: only the argument checks are reached)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError, match="cap"):
            binding.Context.stream_inspect_select(ctx, bad)
    with pytest.raises(ValueError, match="does not fit"):
        binding.Context.stream_inspect_select(ctx, 4, servant=-1)
    with pytest.raises(ValueError, match="page"):
        next(streaming.iter_tasks(ctx, 0))


def test_the_predicate_swept_under_sanitizers(tmp_path):
    """Includes only lease_filter.h; built the way the sanitizer programs of the Makefile are, and run
    as a program of its own: all 2^9 combinations of the predicates on edge values."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "lease_filter_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "lease_filter_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "LEASE-FILTER-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
