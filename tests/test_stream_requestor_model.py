"""The model of the load per requestor (tests/stream_requestor_model.py) without a GPU: its fold
against a dictionary count on the states of the inspection model, the closed form of the admission
clip against the sequential loop, the stand-alone sanitizer program over admit_clip.h, and the
Python surface (dtype, symbols, the printed table)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import stream_inspect_model as IM
from tests import stream_lease_model as L
from tests import stream_outlook_model as OM
from tests import stream_requestor_model as QM
from tests import stream_rpc_model as RM
from tests import stream_wait_lease_model as WM
from tests.conftest import ROOT
from yadcc_amd import binding, streaming, synth


def load_rows(leases, waiting_rows):
    out = np.zeros(len(leases), QM.DTYPE)
    out["leases"], out["waiting_rows"] = leases, waiting_rows
    return out


def same_clip(ip, imm, pre, load, cap):
    a, b = QM.admit_clip(ip, imm, pre, load, cap), QM.admit_clip_closed(ip, imm, pre, load, cap)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (ip, imm, pre, load, cap, a, b)
    return a


def test_closed_form_equals_the_loop_on_random_cases():
    rng = np.random.default_rng(11)
    kinds = dict(room0=0, plenty=0, one=0, distinct=0, zeros=0)
    for case in range(10000):
        n = int(rng.integers(1, 9))
        kind = case % 5
        if kind == 2:
            ip = np.full(n, 7, np.uint32)  # one requestor only
        elif kind == 3:
            ip = rng.permutation(64)[:n].astype(np.uint32)  # all distinct
        else:
            ip = rng.integers(0, 3, n).astype(np.uint32)
        imm, pre = rng.integers(0, 6, n).astype(np.uint32), rng.integers(0, 6, n).astype(np.uint32)
        if kind == 4:
            imm[rng.random(n) < 0.5] = 0  # wants of 0
            pre[imm == 0] = 0
        cap = int(rng.integers(0, 24))
        held = {int(k): (int(rng.integers(0, 30)), int(rng.integers(0, 10))) for k in set(ip.tolist())}
        if kind == 0:
            held = {k: (cap, 0) for k in held}  # room 0
        if kind == 1:
            cap, held = 1000, {k: (0, 0) for k in held}  # room >= total
        load = load_rows([held[int(k)][0] for k in ip], [held[int(k)][1] for k in ip])
        use_pre = None if case % 7 == 0 else pre
        got_imm, got_pre = same_clip(ip, imm, use_pre, load, cap)
        if kind == 0:
            assert not got_imm.any() and not got_pre.any()
        if kind == 1:
            assert np.array_equal(got_imm, imm) and np.array_equal(got_pre, pre if use_pre is not None else 0 * pre)
        kinds[list(kinds)[kind]] += 1
        for k in set(ip.tolist()):  # nobody gets beyond its room, nobody is short-changed below it
            mine = ip == k
            room = max(cap - sum(held[int(k)]), 0)
            want = int(imm[mine].sum()) + (int(pre[mine].sum()) if use_pre is not None else 0)
            assert int(got_imm[mine].sum()) + int(got_pre[mine].sum()) == min(want, room)
    assert all(v == 2000 for v in kinds.values())


def test_clip_by_hand():
    one = np.zeros(3, np.uint32) + 5
    # The cap is reached in the middle of the second row: 4 held, cap 10 -> room 6; rows want 4, 4, 4.
    imm, pre = same_clip(one, [4, 4, 4], [0, 0, 0], load_rows([3, 3, 3], [1, 1, 1]), 10)
    assert imm.tolist() == [4, 2, 0] and pre.tolist() == [0, 0, 0]
    # Prefetch is clipped before immediate: room 5 for a row of 3 + 4, then nothing is left.
    imm, pre = same_clip(one[:2], [3, 1], [4, 0], load_rows([5, 5], [0, 0]), 10)
    assert imm.tolist() == [3, 0] and pre.tolist() == [2, 0]
    # ... and inside one row the immediate grants go first even when they alone are too many.
    imm, pre = same_clip(one[:1], [7], [2], load_rows([5], [0]), 10)
    assert imm.tolist() == [5] and pre.tolist() == [0]
    # Outstanding > cap: room 0, not a negative number. Zombies are inside leases already.
    imm, pre = same_clip(one[:2], [1, 2], [1, 0], load_rows([8, 8], [9, 9]), 10)
    assert not imm.any() and not pre.any()
    # Two requestors interleaved never interact.
    ip = np.array([1, 2, 1, 2], np.uint32)
    imm, pre = same_clip(ip, [3, 3, 3, 3], None, load_rows([0, 6, 0, 6], [0, 0, 0, 0]), 8)
    assert imm.tolist() == [3, 2, 3, 0] and not pre.any()
    with pytest.raises(ValueError):
        QM.admit_clip(one[:1], [1], None, load_rows([QM.UNKNOWN], [0]), 10)


def dictionary_count(tasks, waiting):
    rows, un = {}, 0
    if tasks is not None:
        for k in range(len(tasks["task_id"])):
            if int(tasks["started_at"][k]) == IM.NO_TIME:
                un += 1
                continue
            r = rows.setdefault(int(tasks["requestor_ip"][k]), [0, 0, 0, 0, 0])
            r[0] += 1
            r[1] += int(tasks["zombie"][k] != 0)
            r[2] += int(tasks["prefetch"][k])
    if waiting is not None:
        for k in range(len(waiting["tag"])):
            r = rows.setdefault(int(waiting["requestor_ip"][k]), [0, 0, 0, 0, 0])
            r[3] += 1
            r[4] += int(waiting["n_immediate"][k]) + int(waiting["n_prefetch"][k])
    return rows, un


@pytest.mark.parametrize("mode", ["leased", "wait_leased", "rpc"])
def test_fold_equals_a_dictionary_count_on_the_inspection_models_states(mode):
    # (tight enough in the modes with a queue that requests wait and are granted later)
    sv = synth.make_servants(48, n_tasks_hint=400 if mode == "leased" else 100, n_envs=2, seed=3)
    if mode == "leased":
        M, ws = L, L.LeaseStream(sv, 60, 40, 8, L.LeaseTable(), n_envs=2, report_frac=0.3)
    elif mode == "wait_leased":
        M, ws = WM, WM.new_stream(sv, 60, 40, 8, 300, n_envs=2, rate=lambda now: 1.0 if now % 6 < 4 else 0.25, report_frac=0.3)
    else:
        M, ws = RM, RM.new_stream(sv, 12, 40, 8, 200, 600, n_envs=2, report_frac=0.3,
                                  rate=lambda now: 1.0 if now % 6 < 4 else 0.25)
    ws.es.hb = 12
    I = None
    seen = dict(zombies=0, waiting=0, prefetch=0, unattributed=0, leases=0)
    for t in range(16):
        if t == 3:  # (the leases of the first ticks stay without a record)
            I = IM.attach(ws)
        ev = ws.next_tick()
        if I is None:
            M.model_tick(ws, ev)
        else:
            IM.model_tick(M, ws, ev)
        got, un = QM.stream_fold(ws, I)
        tasks = None if I is None else I.tasks()
        waiting = None if mode == "leased" else OM.stream_waiting(ws)
        want, want_un = dictionary_count(tasks, waiting)
        assert got["requestor_ip"].tolist() == sorted(want), t
        assert (np.diff(got["requestor_ip"].astype(np.int64)) > 0).all()
        if I is None:
            assert un == QM.UNKNOWN and (got["leases"] == QM.UNKNOWN).all() and (got["zombies"] == QM.UNKNOWN).all()
            assert [list(map(int, (r["waiting"], r["waiting_rows"]))) for r in got] == [want[int(r["requestor_ip"])][3:] for r in got]
            continue
        assert un == want_un
        for r in got:
            assert [int(r[k]) for k in QM.COLUMNS] == want[int(r["requestor_ip"])], (t, r)
        # find: a hit echoes the row, a miss is zeros, queries may repeat
        q = np.concatenate([got["requestor_ip"][:3], [0, 0xFFFFFFFF], got["requestor_ip"][:1]]).astype(np.uint32)
        f = QM.find(got, q)
        for i, ip in enumerate(q.tolist()):
            assert int(f["requestor_ip"][i]) == ip
            assert [int(f[k][i]) for k in QM.COLUMNS] == want.get(ip, [0] * 5)
        seen["zombies"] += int(got["zombies"].sum())
        seen["waiting"] += int(got["waiting"].sum())
        seen["prefetch"] += int(got["prefetch_leases"].sum())
        seen["unattributed"] += un
        seen["leases"] += int(got["leases"].sum())
    assert seen["leases"] and seen["zombies"] and seen["unattributed"], seen
    assert (seen["waiting"] > 0) == (mode != "leased") and (seen["prefetch"] > 0) == (mode == "rpc"), seen


def test_admit_clip_header_under_sanitizers(tmp_path):
    """tests/native/admit_clip_test.cc includes only admit_clip.h; built the way the sanitizer programs
    of tests/native/Makefile are, and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "admit_clip_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "admit_clip_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ADMIT-CLIP-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


def test_python_surface():
    assert binding.REQUESTOR_DTYPE == QM.DTYPE and binding.REQUESTOR_DTYPE.itemsize == 24
    assert binding.REQUESTOR_UNKNOWN == QM.UNKNOWN
    for name in ("ydc_stream_requestor_find", "ydc_stream_requestor_get", "ydc_admit_clip"):
        assert name in binding.ABI_SYMBOLS
    assert callable(binding.Context.stream_requestor_find) and callable(binding.Context.stream_requestors)
    assert callable(binding.admit_clip) and callable(streaming.admit)
    assert "REQUESTOR_COMBINE" in binding._TUNE_KEYS
    load = np.zeros(3, QM.DTYPE)
    load["requestor_ip"] = [2, 9, 0xFFFFFFFF]
    load["leases"], load["zombies"], load["prefetch_leases"] = [5, QM.UNKNOWN, 1], [1, QM.UNKNOWN, 0], [0, QM.UNKNOWN, 1]
    load["waiting"], load["waiting_rows"] = [0, 4, 0], [0, 11, 0]
    lines = streaming.requestor_table(load, {2: "10.0.0.2", 0xFFFFFFFF: "255.255.255.255"}).splitlines()
    assert lines[0].split() == ["requestor", "leases", "zombies", "prefetch_leases", "waiting", "waiting_rows"]
    assert lines[1].split() == ["10.0.0.2", "5", "1", "0", "0", "0"]
    assert lines[2].split() == ["#9", "-", "-", "-", "4", "11"] and lines[3].split()[0] == "255.255.255.255"
    assert streaming.requestor_table(load[:1], ["a", "b", "c"]).splitlines()[1].split()[0] == "c"
