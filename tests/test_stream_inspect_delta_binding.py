"""ydc_stream_delta_inspect / ydc_stream_inspect_restore / ydc_stream_delta_apply_inspected without a GPU:
the header declares the three entry points with the signatures the binding types, the library exports
them, and none of them touches a device before it has looked at its arguments. Every test fails without
the feature: the symbols are missing."""
import ctypes as C
import os
import re
import subprocess

from tests.conftest import ROOT
from yadcc_amd import binding, snapshot, streaming

HEADER = os.path.join(ROOT, "include", "yadcc_dispatch.h")
DECLARED = {
    "ydc_stream_delta_inspect": ["ydc_context* ctx", "const void* delta", "size_t delta_bytes", "void* out", "size_t cap",
                                 "size_t* out_bytes"],
    "ydc_stream_inspect_restore": ["ydc_context* ctx", "const void* side", "size_t bytes"],
    "ydc_stream_delta_apply_inspected": ["ydc_context* ctx", "const void* delta", "size_t delta_bytes", "const void* side",
                                         "size_t side_bytes"],
}
CTYPE = {"ydc_context*": C.c_void_p, "const void*": C.c_char_p, "void*": C.c_void_p, "size_t": C.c_size_t,
         "size_t*": C.POINTER(C.c_size_t)}


def test_the_header_declares_what_the_binding_types():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, params in DECLARED.items():
        m = re.search(r"\bint %s\((.*?)\);" % name, src, re.S)
        assert m, "%s is not declared" % name
        got = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert got == params, (name, got)
        want = [CTYPE[p.rsplit(" ", 1)[0]] for p in params]
        assert getattr(binding.lib(), name).argtypes == want, name
    assert re.search(r"#define YDC_ABI_VERSION 8u\b", src) and binding.ABI_VERSION == 8  # (additive: it does not move)


def test_symbols_methods_and_wrappers():
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "lib"], cwd=ROOT)
    lib = C.CDLL(binding.LIB_PATH)
    for name in DECLARED:
        assert name in binding.ABI_SYMBOLS and hasattr(lib, name), name
    for method in ("stream_delta_inspect", "stream_inspect_restore", "stream_delta_apply_inspected"):
        assert callable(getattr(binding.Context, method))
    for fn in (streaming.standby_base, streaming.standby_restore, streaming.standby_step, snapshot.parse_inspect_delta,
               snapshot.build_inspect_delta, snapshot.apply_inspect_delta):
        assert callable(fn)
    assert binding.lib().ydc_strerror(-1) == b"invalid argument"  # (no new error code: the refusals are this one)


def test_no_call_touches_a_device_before_its_arguments():
    L = binding.lib()
    need = C.c_size_t(7)
    buf = C.create_string_buffer(b"\xAA" * 256, 256)
    blob = bytes(200)
    assert L.ydc_stream_delta_inspect(None, None, 0, buf, 256, C.byref(need)) == -1 and need.value == 7
    assert L.ydc_stream_delta_inspect(None, blob, len(blob), buf, 256, C.byref(need)) == -1
    assert buf.raw == b"\xAA" * 256
    assert L.ydc_stream_inspect_restore(None, blob, len(blob)) == -1
    assert L.ydc_stream_delta_apply_inspected(None, blob, len(blob), blob, len(blob)) == -1
