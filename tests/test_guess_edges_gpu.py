"""The start states of k_match_pass, on the device: the cases of tests/guess_edge_cases.py (verified
on the CPU by tests/test_guess_edges_model.py) through ydc_dispatch.

Exact pools (the level guess is the true start state): placement, utilisation and running_tasks
EQUAL the oracle's, and with YDC_DEBUG_SIM=1 the kernel's replay counter says that NO chunk was
replayed twice — chunk_sims == n_chunks — in the fused form (pass 0 + 1 in one launch, with
warm-ups: two rounds, because a warmed-up pass 0 certifies nothing) and with YDC_FUSE_PASSES=0
(pass 0 certifies itself: one round). A wrong level-table lookup, quartile probe, search window,
tail count or warm-up start shows as a second replay. The control pools (own hosts) prove that
the counter moves.

Walk pools (YDC_ZONE_GUESS=2): equality with the oracle, zone_rows == the restated z_hi - z_lo (0
where the restatement or the plan finds no zone), and — one child process on the measurement
build — the header words (T0, z_lo, z_hi, t_start) and EVERY cursor of EVERY row the walk
published equal the Python restatement, which the CPU test has shown to be the truth.

Rounds, replays and rows of one run on an MI355X are in the docstrings below. Wall time of the
whole file there, measured once: 5.2 s for its 98 tests (1.4 s of them the child process on the
measurement build, which was built beforehand)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (the probe child runs this file as a program)
    sys.path.insert(0, ROOT)

from oracle import oraclebind as O  # noqa: E402
from tests import guess_edge_cases as G  # noqa: E402
from yadcc_amd import binding, pack  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT = G.exact_cases() + G.disjoint_cases()
CONTROL = G.control_cases()
WALK = G.walk_cases()
ids = lambda cases: [c.name for c in cases]


@functools.lru_cache(maxsize=None)
def staged(name):
    """[(servants, requests, the oracle's answer)] of a case's batches."""
    return [(sv, tk, O.dispatch(sv, tk, "scan")) for sv, tk in G.stages(G.case(name))]


def run_case(case, setenv, **extra):
    """Every batch of the case, committed, on one context: each equal to the oracle. Returns the
    (stats, kernel profile) of every batch."""
    for k, v in dict(case.switches, DEBUG_SIM=1, **extra).items():
        setenv("YDC_" + k, str(v))
    stages = staged(case.name)
    c = binding.Context(device=0)
    out = []
    try:
        c.set_profiling(True)
        c.upload_servants(pack.to_abi_columns(stages[0][0]))
        for sv, tk, (want, wutil, wrun) in stages:
            got, gutil, grun = c.dispatch(tk, commit=True)
            st = c.stats()
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (case, bad[:5], got[bad[:5]], want[bad[:5]], st)
            assert np.array_equal(gutil, wutil) and np.array_equal(grun, wrun), case
            assert np.array_equal(c.get_running(), wrun), case
            assert st["small_batch"] == 0 and st["n_classes"] == case.promise["C"], (case, st)
            assert st["n_chunks"] == -(-len(want) // case.cs), (case, st)
            out.append((st, c.kernel_profile()))
    finally:
        c.close()
    return out


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "pass-0-alone"])
@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_exact_pool_no_chunk_is_replayed_twice(case, fuse, monkeypatch):
    """One run on an MI355X: chunk_sims == n_chunks (32 .. 128) in all 60 runs and in both batches
    of the cut cases; fused: 2 rounds wherever the plan warms up, 1 for k_guess_init, more than 64
    classes and disjoint digests; pass 0 alone: 1 round everywhere. No 3 was seen (no hand-over wait
    ran out)."""
    plan = G.guess_plan(case.data()[0], len(case.data()[1]["env_id"]), n_parts=case.promise.get("parts", 1),
                        **dict({k.lower(): int(v) for k, v in case.switches.items()}, fuse_passes=fuse))
    assert plan["form"] == case.path
    for st, prof in run_case(case, monkeypatch.setenv, FUSE_PASSES=fuse):
        print(case.name, "fused" if fuse else "pass 0 alone", "n_chunks", st["n_chunks"], "chunk_sims", st["chunk_sims"],
              "rounds", st["rounds"])
        assert ("k_bin_sort" in prof) == plan["binsort"], (case, sorted(prof))
        assert ("k_guess_init" in prof) == (case.path == G.INIT), (case, sorted(prof))
        assert st["chunk_sims"] == st["n_chunks"], (case, st)
        if fuse:  # (3: a hand-over wait ran out — a finding to write down, not an error)
            assert st["rounds"] in (plan["rounds"], 3), (case, st)
        else:
            assert st["rounds"] == 1, (case, st)


@pytest.mark.parametrize("case", CONTROL, ids=ids(CONTROL))
def test_control_pool_moves_the_replay_counter(case, monkeypatch):
    """A tenth of the requests, the last of every chunk among them, come from the host of the servant
    at the head: the chunk hands a state with a hole to its successor, which no level guess has.
    Pass 0 alone must replay such successors again. (The fused form is printed, not asserted: a
    warm-up that starts in front of the own-host request steps over the same slot and arrives at the
    very state its predecessor ends in — that it heals holes is what it is for.) One run on an
    MI355X: 115 .. 122 replays of 64 chunks with pass 0 alone; fused 64 of 64, and 122 for
    k_guess_init, which has no warm-up."""
    for st, _ in run_case(case, monkeypatch.setenv, FUSE_PASSES=0):
        print(case.name, "pass 0 alone: n_chunks", st["n_chunks"], "chunk_sims", st["chunk_sims"], "rounds", st["rounds"])
        assert st["chunk_sims"] > st["n_chunks"] and st["rounds"] > 1, (case, st)
    for st, _ in run_case(case, monkeypatch.setenv, FUSE_PASSES=1):
        print(case.name, "fused: n_chunks", st["n_chunks"], "chunk_sims", st["chunk_sims"], "rounds", st["rounds"])


@functools.lru_cache(maxsize=None)
def restated(name):
    case = G.case(name)
    sv, tk = G.stages(case)[-1]
    n = len(tk["env_id"])
    plan = case.plan(n)
    z = G.zone_restate(sv, tk, case.cs, case.promise["lead"], case.promise["trail"], plan["warm_len"])
    return plan, z


@pytest.mark.parametrize("case", WALK, ids=ids(WALK))
def test_walk_serves_the_restated_chunks(case, monkeypatch):
    """Product build: zone_rows == the restated z_hi - z_lo. And two runs more without an assertion:
    rounds and replays with the walk and without it."""
    plan, z = restated(case.name)
    assert plan["walk"] == (case.path == "walk")
    st, prof = run_case(case, monkeypatch.setenv)[-1]
    assert "k_bin_sort" not in prof and "k_guess_init" not in prof, sorted(prof)
    assert st["zone_rows"] == (z["rows"] if plan["walk"] else 0), (case, st, z["z_lo"], z["z_hi"])
    off, _ = run_case(case, monkeypatch.setenv, ZONE_GUESS=0)[-1]
    assert off["zone_rows"] == 0
    print("%s: zone_rows %d of %d chunks | with the walk: rounds %d, chunk_sims %d | without: rounds %d, chunk_sims %d"
          % (case.name, st["zone_rows"], st["n_chunks"], st["rounds"], st["chunk_sims"], off["rounds"], off["chunk_sims"]))


# ---------------------------------------------------------------------------------------------
# The walk's header and cursors, from the measurement build
# ---------------------------------------------------------------------------------------------
def _probe_child():
    """Runs in a process of its own on the measurement build (YDC_LIB): every walk case, checked
    against the oracle, then words 60000 .. 60003 and 60008 + row * 64 + class of the phase probe."""
    import ctypes as C
    L = binding.lib()
    L.ydc_debug_phase_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    L.ydc_debug_phase_probe.restype = C.c_int
    out = {}
    for case in WALK:
        mine = dict(case.switches)
        for k, v in mine.items():
            os.environ["YDC_" + k] = str(v)
        stages = [(sv, tk, O.dispatch(sv, tk, "scan")) for sv, tk in G.stages(case)]
        c = binding.Context(device=0)
        c.upload_servants(pack.to_abi_columns(stages[0][0]))
        for sv, tk, (want, wutil, wrun) in stages:
            assert L.ydc_debug_phase_probe(None, 0, 1) == 0
            got, gutil, grun = c.dispatch(tk, commit=True)
            assert np.array_equal(got, want) and np.array_equal(gutil, wutil) and np.array_equal(grun, wrun), case
        buf = np.zeros(60008 + G.ZONE_MAX_ROWS * 64, np.uint64)
        assert L.ydc_debug_phase_probe(buf.ctypes.data, buf.size, 0) == 0
        rows = c.stats()["zone_rows"]
        c.close()
        for k in mine:
            del os.environ["YDC_" + k]
        cur = buf[60008:].reshape(G.ZONE_MAX_ROWS, 64)[:rows, :case.promise["C"]]
        out[case.name] = dict(header=[int(x) for x in buf[60000:60004]], rows=rows, cursors=cur.astype(np.int64).tolist())
    print("PROBE " + json.dumps(out))


def test_walk_publishes_the_restated_cursors():
    """One run on an MI355X: the four header words of all 30 cases and all 4810 cursors of the 23
    walks of two rows or more (4 .. 32 rows of 9 .. 64 classes) equal the restatement."""
    subprocess.check_call(["make", "-s", "probe"], cwd=ROOT)
    env = dict(os.environ, YDC_LIB=os.path.join(ROOT, "yadcc_amd", "libydc_probe.so"))
    env.pop("YDC_TUNE", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "probe"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("PROBE ")][-1]
    seen = json.loads(line[len("PROBE "):])
    compared = 0
    for case in WALK:
        plan, z = restated(case.name)
        got = seen[case.name]
        if not plan["walk"]:
            want_header = [0, 0, 0, 0]  # (no walk was launched: nothing is stamped)
        elif z["rows"] == 0:
            want_header = [z["T0"], 0, 0, 0]
        else:
            want_header = [z["T0"], z["z_lo"], z["z_hi"], z["t_start"]]
        print(case.name, "header", got["header"], "rows", got["rows"], "cursors compared",
              len(z["cursors"]) * plan["C"] if plan["walk"] else 0)
        assert got["header"] == want_header, (case, got["header"], want_header)
        assert got["rows"] == (z["rows"] if plan["walk"] else 0), (case, got["rows"], z["rows"])
        if plan["walk"] and z["rows"] >= 2:
            mine, theirs = np.array(z["cursors"]), np.array(got["cursors"])
            assert mine.shape == theirs.shape, (case, mine.shape, theirs.shape)
            bad = np.argwhere(mine != theirs)
            assert bad.size == 0, (case, bad[:5], mine[tuple(bad[0])], theirs[tuple(bad[0])])
            compared += mine.size
    want = sum(z["cursors"].size for plan, z in map(restated, ids(WALK)) if plan["walk"] and z["rows"] >= 2)
    assert compared == want > 0, (compared, want)
    print("cursors compared in all:", compared)


if __name__ == "__main__":
    if sys.argv[1:] == ["probe"]:
        _probe_child()
