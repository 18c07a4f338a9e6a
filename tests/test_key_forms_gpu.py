"""The closed forms of dispatch_core.h on the device: tests/native/key_forms_gpu evaluates
slot_key_exact, slot_key_fp64, first_slot_not_below / _direct / _direct32 and servant_slots_before
(exact and fp64 keys) for 2 * 10^5 cases of tests/key_edge_cases.py — servants of the edge
families, thresholds that ARE keys of slots, and those +- 1 — one thread per case. Every output is
compared with integer references; the fp64 key with numpy's float64 division, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import key_edge_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "native", "key_forms_gpu")


def test_closed_forms_on_the_device(tmp_path):
    assert os.path.exists(PROGRAM), "tests/native/key_forms_gpu is missing: `make native`"
    tab = K.key_form_cases(200_000, seed=3)
    ref, ok32 = K.key_form_reference(tab)
    assert 3 * int(ok32.sum()) >= len(tab)  # the 32-bit form runs on at least a third
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    tab.tofile(src)
    p = subprocess.run([PROGRAM, src, dst], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout[-2000:]
    out = np.fromfile(dst, K.FORM_OUT_DTYPE)
    assert len(out) == len(tab)
    assert int((out["first_direct32"] != K.FORM_NOT_RUN).sum()) == int(ok32.sum())
    for name in K.FORM_OUT_DTYPE.names:
        diff = np.nonzero(out[name] != ref[name])[0]
        assert diff.size == 0, (name, diff.size, tab[diff[:3]], out[name][diff[:3]], ref[name][diff[:3]])
