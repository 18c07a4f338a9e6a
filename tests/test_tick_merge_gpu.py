"""k_tick (yadcc_amd/csrc/tick_kernel.h) where the other tick tests do not reach: the merge that
places the identical requests of one RPC (tick_merges, build_list, the round loop) and the
resident kernel's mailbox (TickBox, tick_run, the poll loop) carrying real deltas.

Every turn is checked against the literal restatement of the reference (oracle "scan") on a host
copy of the registry that replays the turn's heartbeat rows and released grants first: integer
equality on placements, the same doubles on utilisations, the granted / timeouts / env_not_found
counters. running_tasks is compared with get_running() only at checkpoints — that call ends the
resident kernel; between checkpoints a wrong running_tasks shows in the following answers.

`Turns` keeps a model of which commands the one-workgroup kernel takes (the thresholds of
ydc_context::small_batch and tick_takes) and of the resident kernel's life (what launches one,
what ends one), and after every turn asserts stats()["small_batch"], tick_resident_calls and
tick_launched_calls against it: a resident sequence proves that it was resident.

Register widths by registry size: 256 threads x 1, 2, 4, 8, 16 servants up to 256, 512, 1024,
2048, 4096 servants; 512 x 16 up to 8192; 512 x 32 (columns re-read by the owner) beyond."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (the witness child runs this file as a program)
    sys.path.insert(0, ROOT)

from oracle import oraclebind as O  # noqa: E402
from yadcc_amd import binding, pack, synth  # noqa: E402

pytestmark = pytest.mark.gpu

GIB = 1 << 30
FOREIGN = 0xAC100001  # 172.16.0.1: a host that runs no servant (servants live in 10.0.0.0/8)
ENF, TIMEOUT = O.IDX_ENV_NOT_FOUND, O.IDX_TIMEOUT

# (key format, want_util): the one-word candidate, the reference's double, and the double with the
# chosen servants' utilisations (which the merge computes only there)
MODES = [("1", False), ("0", False), ("0", True)]
MODE_IDS = ["packed", "fp64", "fp64-util"]


def _threads(S):
    return 256 if S <= 4096 else 512


def _rpc(n, env=0, minv=0, rip=FOREIGN):
    return {"env_id": np.full(n, env, np.uint32), "min_version": np.full(n, minv, np.uint32),
            "requestor_ip": np.full(n, rip, np.uint32)}


def _pool(S, seed, n_envs=3):
    """A random pool with capacities up to 243 (the packed key holds them up to 16384 servants),
    about half full."""
    sv = synth.make_servants(S, n_envs=n_envs, seed=seed)
    sv = {k: np.array(v, copy=True) for k, v in sv.items()}
    rng = np.random.default_rng(seed + 1)
    top = np.minimum(sv["max_tasks"], sv["num_processors"]).astype(np.int64)
    sv["running_tasks"] = (rng.random(S) * (top + 2)).astype(np.uint32)
    assert int(top.max()) <= 255
    return sv


def _flat_pool(S, nproc=64, max_tasks=40, running=None):
    """Hand-made: user servants of one digest, version 20, no foreign load, each on its own host;
    by default loaded to 70 .. 85 % (clearly worse than whatever a case plants among them)."""
    if running is None:
        running = 28 + np.arange(S) % 7
    return {
        "version": np.full(S, 20, np.uint32),
        "num_processors": np.full(S, nproc, np.uint32),
        "current_load": np.zeros(S, np.uint32),
        "max_tasks": np.full(S, max_tasks, np.uint32),
        "running_tasks": np.broadcast_to(np.asarray(running, np.uint32), (S,)).copy(),
        "priority": np.full(S, synth.PRIORITY_USER, np.uint32),
        "total_memory": np.full(S, 64 * GIB, np.uint64),
        "memory_available": np.full(S, 32 * GIB, np.uint64),
        "env_mask": np.ones(S, np.uint64),
        "ip": ((10 << 24) + 1 + np.arange(S)).astype(np.uint32),
        "port": np.full(S, 8335, np.uint32),
    }


def _rows(sv, idx):
    idx = np.asarray(idx, np.int64)
    rows = np.zeros(len(idx), binding.ROW_DTYPE)
    flags = pack.servant_flags(sv)
    for k, col in (("version", "version"), ("num_processors", "num_processors"), ("current_load", "current_load"),
                   ("max_tasks", "max_tasks"), ("ip_id", "ip"), ("env_mask", "env_mask")):
        rows[k] = np.asarray(sv[col])[idx]
    rows["flags"] = flags[idx]
    return rows


def _tick_limit(S, same, packed):
    """ydc_context::small_batch with the default threshold; `same` counts with one-word candidates
    only (tick_takes)."""
    return 64 if (S <= 4096 or (same and packed)) else 48 if S <= 8192 else 32


def _is_same(tk):
    n = len(tk["env_id"])
    return n >= 2 and all(bool((tk[k] == tk[k][0]).all()) for k in ("env_id", "min_version", "requestor_ip"))


class Turns:
    """One context, its host copy of the registry, the grants it holds, and the model of the
    resident kernel's life."""

    def __init__(self, sv, packed, want_util=False):
        self.sv = {k: np.array(v, copy=True) for k, v in sv.items()}
        self.S = len(self.sv["version"])
        self.packed, self.want_util = packed, want_util
        self.c = binding.Context(device=0)
        self.c.upload_servants(pack.to_abi_columns(self.sv))
        self.held = []
        self.alive = False  # a resident kernel is waiting at its mailbox
        self.alive_util = False
        st = self.c.stats()
        self.resident, self.launched = st["tick_resident_calls"], st["tick_launched_calls"]
        self.commands = self.mailbox = 0

    def close(self):
        self.c.close()

    def reset(self, running):
        """Another initial load for the same registry (ends the resident kernel)."""
        self.sv["running_tasks"] = np.array(running, np.uint32, copy=True)
        self.c.set_running(self.sv["running_tasks"])
        self.alive = False
        self.held = []

    def release(self, rng, n):
        """n of the held grants, chosen at random (a servant may come several times)."""
        return [self.held.pop(int(rng.integers(len(self.held)))) for _ in range(min(n, len(self.held)))]

    def turn(self, tk, upd_idx=(), rel=(), commit=True, want_util=None, where=None):
        """One ydc_dispatch_tick. The heartbeat rows are what self.sv holds for upd_idx (the caller
        has changed those columns); returns the oracle's placements."""
        sv, c = self.sv, self.c
        wu = self.want_util if want_util is None else want_util
        upd_idx = np.asarray(upd_idx, np.uint32)
        for s in rel:
            sv["running_tasks"][s] -= 1
        n = len(tk["env_id"])
        want, wutil, wrun = O.dispatch(sv, tk, "scan")
        got, gutil = c.dispatch_tick(tk, upd_idx, _rows(sv, upd_idx), rel, commit=commit, want_util=wu)
        st = c.stats()
        ctx = (where, n, len(upd_idx), len(rel), st)
        assert np.array_equal(got, want), (ctx, got, want)
        if wu:
            assert np.array_equal(gutil, wutil), (ctx, gutil, wutil)
        takes = n <= _tick_limit(self.S, _is_same(tk), self.packed)
        if n:
            assert st["small_batch"] == int(takes), ctx
            assert st["granted"] == int((want < ENF).sum()), ctx
            assert st["timeouts"] == int((want == TIMEOUT).sum()), ctx
            assert st["env_not_found"] == int((want == ENF).sum()), ctx
        # the resident kernel's life: a COMMITting command within what the mailbox holds is taken
        # by the kernel that waits there (same kind of answer), or launches the one that stays
        if takes:
            stays = commit and len(upd_idx) <= 16 and len(rel) <= 64
            if self.alive and stays and self.alive_util == wu:
                self.resident += 1
                self.mailbox += 1
            else:
                self.launched += 1
                self.alive, self.alive_util = stays, wu
            self.commands += 1
        else:
            self.alive = False  # (the batch pipeline ends it first)
        assert (st["tick_resident_calls"], st["tick_launched_calls"]) == (self.resident, self.launched), ctx
        if commit:
            sv["running_tasks"] = wrun
            self.held.extend(int(s) for s in got if s < ENF)
        return want

    def checkpoint(self, where=None):
        got = self.c.get_running()
        self.alive = False
        assert np.array_equal(got, self.sv["running_tasks"]), (where, np.nonzero(got != self.sv["running_tasks"])[0][:8])


@pytest.fixture(params=MODES, ids=MODE_IDS)
def mode(monkeypatch, request):
    packed, want_util = request.param
    monkeypatch.setenv("YDC_PACKED_TICK", packed)
    # (the idle exit has its own test: here a slow host must not end a life that is counted)
    monkeypatch.setenv("YDC_RESIDENT_IDLE_MS", "20000")
    return packed == "1", want_util


@pytest.fixture(params=MODES[:2], ids=MODE_IDS[:2])
def key_mode(monkeypatch, request):
    monkeypatch.setenv("YDC_PACKED_TICK", request.param[0])
    monkeypatch.setenv("YDC_RESIDENT_IDLE_MS", "20000")
    return request.param[0] == "1"


# ---------------------------------------------------------------------------------------------
# 1. The merge at every register width
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [200, 400, 900, 1500, 3000, 6000, 12000])
def test_merge_at_every_register_width(S, mode):
    """K = 1, 2, 4, 8, 16, 512 x 16, 512 x 32; n = 2 (below kTickMergeMin), 3, 63, 64; both version
    thresholds: in ONE resident kernel three identical RPCs, a call of distinct requests, the RPC
    again. Past 4096 servants the fp64 key places 63 / 64 identical requests with the batch
    pipeline (the model in Turns says which), and a kernel then begins a new life."""
    packed, want_util = mode
    sv = _pool(S, seed=100 + S)
    t = Turns(sv, packed, want_util)
    try:
        for n in (2, 3, 63, 64):
            for minv in (0, 20):
                t.reset(sv["running_tasks"])
                rpc = _rpc(n, env=0, minv=minv, rip=FOREIGN + n)
                distinct = synth.make_tasks(9, sv, n_envs=3, seed=S + n + minv, self_frac=0.3)
                before = t.mailbox
                takes = n <= _tick_limit(S, True, packed)
                for step, tk in enumerate((rpc, rpc, rpc, distinct, rpc)):
                    t.turn(tk, where=(S, n, minv, step))
                t.checkpoint((S, n, minv))
                assert t.mailbox - before == (4 if takes else 0), (S, n, minv)
    finally:
        t.close()


@pytest.mark.parametrize("S", [6000, 12000])
def test_routing_of_identical_requests_past_4096_servants(S, monkeypatch):
    """With one-word candidates 64 identical requests take the tick kernel and 64 distinct ones do
    not; with the fp64 key 49 identical requests at 6000 servants do not either (tick_takes,
    small_batch(same))."""
    sv = _pool(S, seed=100 + S)
    distinct = synth.make_tasks(64, sv, n_envs=3, seed=3, self_frac=0.0)
    assert not _is_same(distinct)
    monkeypatch.setenv("YDC_PACKED_TICK", "1")
    t = Turns(sv, True)
    try:
        t.turn(_rpc(64, minv=20), where="64 identical")
        assert t.c.stats()["small_batch"] == 1
        t.turn(distinct, where="64 distinct")
        assert t.c.stats()["small_batch"] == 0
        t.checkpoint()
    finally:
        t.close()
    if S == 6000:
        monkeypatch.setenv("YDC_PACKED_TICK", "0")
        t = Turns(sv, False)
        try:
            t.turn(_rpc(48, minv=20), where="48 identical, fp64")
            assert t.c.stats()["small_batch"] == 1
            t.turn(_rpc(49, minv=20), where="49 identical, fp64")
            assert t.c.stats()["small_batch"] == 0
            t.checkpoint()
        finally:
            t.close()


# ---------------------------------------------------------------------------------------------
# 2. Lists that run dry, e1_same, tier crossing, ties
# ---------------------------------------------------------------------------------------------
def _dry_list_pool(S):
    """The best free servants all belong to ONE thread (t0 + j * THREADS), with different
    capacities so that now the same servant, now the runner-up is the thread's second entry."""
    T = _threads(S)
    t0, m = (70, 3) if S <= 4096 else (300, 5)
    mine = [t0 + j * T for j in range(m)]
    sv = _flat_pool(S)
    for j, s in enumerate(mine):
        sv["running_tasks"][s] = 0
        sv["max_tasks"][s] = (60, 50, 44, 56, 48)[j]
    return sv, mine


def _idle_giant_pool(S):
    """One idle servant with 200 free slots among loaded ones."""
    sv = _flat_pool(S)
    s0 = S // 2 + 3
    sv["num_processors"][s0] = sv["max_tasks"][s0] = 200
    sv["running_tasks"][s0] = 0
    return sv, s0


def _tier_crossing_pool(S):
    """Two dedicated servants of one thread a few tasks below 2 * running < nproc, ten lightly
    loaded user servants, everyone else loaded: the dedicated ones win while in tier 0 — at a
    higher utilisation than the light ones — and not once afterwards."""
    T = _threads(S)
    sv = _flat_pool(S)
    d1, d2 = 45, 45 + T
    for s, r in ((d1, 26), (d2, 28)):
        sv["priority"][s] = synth.PRIORITY_DEDICATED
        sv["max_tasks"][s] = 60
        sv["running_tasks"][s] = r
    light = [(7 + 83 * j) % S for j in range(10)]
    assert d1 not in light and d2 not in light
    sv["running_tasks"][light] = 4
    return sv, (d1, d2)


def _tied_pool(S):
    from tests.test_binsort_gpu import _tied_pool as tied
    return {k: np.array(v, copy=True) for k, v in tied(S).items()}


def _run_rpc_life(sv, mode, n, shape, rounds, distinct=True):
    """The RPC `rounds` times, a call of distinct requests behind the first, in one resident kernel;
    `shape(k, want)` asserts on the oracle's k-th answer that the pool does what it was made for.
    (Past 8192 servants the fp64 key leaves more than 32 requests to the batch pipeline: the same
    life again with 32, which the kernel's pick-by-pick loop places.)"""
    packed, want_util = mode
    S = len(sv["version"])
    takes = n <= _tick_limit(S, True, packed)
    for n_req in (n,) if takes else (n, 32):
        t = Turns(sv, packed, want_util)
        try:
            for k in range(rounds):
                shape(k, t.turn(_rpc(n_req), where=("rpc", n_req, k)))
                if k == 0 and distinct:
                    t.turn(synth.make_tasks(5, sv, n_envs=1, seed=9, self_frac=0.4), where="distinct")
            t.checkpoint()
            if n_req <= _tick_limit(S, True, packed):
                assert t.mailbox == t.commands - 1 == rounds - 1 + int(distinct)
            else:
                assert t.mailbox == 0 and t.commands == int(distinct)
        finally:
            t.close()


@pytest.mark.parametrize("S", [900, 12000])
def test_merge_list_runs_dry(S, mode):
    sv, mine = _dry_list_pool(S)

    def shape(k, want):
        assert set(want.tolist()) <= set(mine) and len(set(want.tolist())) >= 3, want
    _run_rpc_life(sv, mode, 40, shape, rounds=2)


@pytest.mark.parametrize("S", [900, 12000])
def test_merge_same_servant_many_times(S, mode):
    sv, s0 = _idle_giant_pool(S)

    def shape(k, want):
        assert (want == s0).all(), want
    _run_rpc_life(sv, mode, 64, shape, rounds=2)


@pytest.mark.parametrize("S", [900, 12000])
def test_merge_tier_crossing(S, mode):
    sv, (d1, d2) = _tier_crossing_pool(S)

    def shape(k, want):
        if k == 0:  # 6 + 4 tasks below half of nproc
            assert set(want[:10].tolist()) == {d1, d2} and not np.isin(want[10:], (d1, d2)).any(), want
            assert (want < ENF).all()
        else:
            assert not np.isin(want, (d1, d2)).any(), want
    _run_rpc_life(sv, mode, 40, shape, rounds=2)


@pytest.mark.parametrize("S", [900, 12000])
def test_merge_ties_first_registered_wins(S, mode):
    """Identical idle servants: 64 requests six times over go to servants 0 .. 383 in order —
    equal keys across lanes, waves and (256 threads) the threads' second servants."""
    sv = _tied_pool(S)

    def shape(k, want):
        assert np.array_equal(want, k * len(want) + np.arange(len(want))), want
    _run_rpc_life(sv, mode, 64, shape, rounds=6, distinct=False)


# ---------------------------------------------------------------------------------------------
# 3. Exhaustion and nobody eligible
# ---------------------------------------------------------------------------------------------
def _exhaustion_pool(S, g):
    """Digest 0 on 30 scattered servants with exactly g free slots in total (two of the free ones
    in one thread), digest 1 on everyone else, digest 2 only on servants that accept no tasks."""
    T = _threads(S)
    sv = _flat_pool(S, nproc=16, max_tasks=8, running=3)
    sv["env_mask"][:] = 0b10
    E = [(11 + 29 * j) % T for j in range(29)]
    E.append(E[3] + T)
    sv["env_mask"][E] = 0b01
    sv["env_mask"][E[20:25]] = 0b11
    sv["running_tasks"][E] = 8
    if g == 1:
        sv["running_tasks"][E[5]] = 7
    elif g == 19:
        sv["running_tasks"][E[3]] = 1
        sv["running_tasks"][E[29]] = 1
        sv["running_tasks"][E[9]] = 3
    none = [S - 1 - 3 * j for j in range(6)]
    assert not set(none) & set(E)
    sv["env_mask"][none] = 0b100
    sv["max_tasks"][none] = 0
    sv["version"][S // 3] = 19
    return sv


@pytest.mark.parametrize("S", [900, 12000])
def test_merge_exhaustion_and_nobody_eligible(S, key_mode):
    """n = 20 against g = 0, 1, 19 free slots (granted first, then IDX_TIMEOUT: stop == 2), a
    digest nobody has, a digest only on max_tasks == 0 servants, min_version above every version
    (20 x IDX_ENV_NOT_FOUND) — launched without COMMIT, and as the second command of a resident
    kernel."""
    nothing = _rpc(0)
    for g in (0, 1, 19):
        sv = _exhaustion_pool(S, g)
        t = Turns(sv, key_mode)
        try:
            cases = [("g=%d" % g, _rpc(20), [0] * g + [TIMEOUT] * (20 - g))]
            if g == 19:
                cases += [("no such digest", _rpc(20, env=5), [ENF] * 20),
                          ("digest on max_tasks == 0 only", _rpc(20, env=2), [ENF] * 20),
                          ("min_version above all", _rpc(20, minv=99), [ENF] * 20)]
            for name, tk, kind in cases:
                def shape(want):
                    assert [int(w) if w >= ENF else 0 for w in want] == kind, (name, want)
                t.reset(sv["running_tasks"])
                shape(t.turn(tk, commit=False, where=(name, "launched")))
                t.checkpoint((name, "launched"))  # (no COMMIT: the column is as it was)
                before = t.mailbox
                t.turn(nothing, where=(name, "empty"))
                shape(t.turn(tk, where=(name, "resident")))
                assert t.mailbox - before == 1
                t.checkpoint((name, "resident"))
        finally:
            t.close()


# ---------------------------------------------------------------------------------------------
# 4. The requestor's own host
# ---------------------------------------------------------------------------------------------
def _own_host_pool(S, case):
    """Servants a and b — the only dedicated ones, idle: the best of the pool for their first 32
    tasks each — and a on the requestor's host."""
    sv = _pool(S, seed=400 + S)
    sv["priority"][:] = synth.PRIORITY_USER
    a, b = S // 3, S // 3 + 7
    for s in (a, b):
        sv["version"][s] = 20
        sv["env_mask"][s] |= np.uint64(1)
        sv["priority"][s] = synth.PRIORITY_DEDICATED
        sv["num_processors"][s], sv["max_tasks"][s] = 64, 60
        sv["current_load"][s] = sv["running_tasks"][s] = 0
        sv["memory_available"][s] = 64 * GIB
    if case == "two":
        sv["ip"][b] = sv["ip"][a]
    elif case == "wrong_digest":
        sv["env_mask"][a] = 0b10
    elif case == "full":
        sv["running_tasks"][a] = 60
    elif case == "only_self_free":
        sv["running_tasks"][:] = 255
        sv["running_tasks"][a] = 0
    return sv, a, b


@pytest.mark.parametrize("case", ["one", "two", "wrong_digest", "full", "only_self_free"])
@pytest.mark.parametrize("S", [200, 1500])
def test_merge_and_the_requestors_own_host(S, case, key_mode):
    """n = 12 at K = 1 and K = 8, one resident kernel: the RPC from a foreign host, from the
    servant's host, from the foreign host, from the servant's host (own-host bits change under
    cached lists). An eligible free servant there abandons the merge; one with another digest or
    without a free slot does not."""
    sv, a, b = _own_host_pool(S, case)
    host = int(sv["ip"][a])
    t = Turns(sv, key_mode)
    try:
        for step, rip in enumerate((FOREIGN, host, FOREIGN, host)):
            want = t.turn(_rpc(12, env=0, minv=20, rip=rip), where=(case, step))
            own = rip == host
            if case == "one":  # `self` is the last resort: the best servant of the pool is passed over
                assert (a in want) == (not own), (step, want)
            elif case == "two":  # the second one on the host competes
                assert (a in want) == (not own) and (b in want or not own), (step, want)
            elif case in ("wrong_digest", "full"):
                assert a not in want and (b in want or step), (step, want)
            else:
                assert (want == a).all(), (step, want)
        t.checkpoint(case)
        assert t.mailbox == 3
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------
# 5. State between commands of one resident kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [900, 12000])
def test_resident_state_scripted(S, key_mode):
    sv = _pool(S, seed=500 + S)
    t = Turns(sv, key_mode)
    rng = np.random.default_rng(S)
    n = 24
    A, A20, B = _rpc(n, env=0, minv=0), _rpc(n, env=0, minv=20), _rpc(n, env=1, minv=0)
    try:
        t.turn(A, where=1)
        t.turn(A, where=2)  # only the threads that were picked from rebuild
        t.turn(synth.make_tasks(9, sv, n_envs=3, seed=S, self_frac=0.2), where=3)  # the loop invalidates the lists
        t.turn(A, where=4)
        t.turn(B, where=5)
        t.turn(A20, where=6)
        # 7: a heartbeat takes the servant A's merge would pick next out of the free ones
        nxt = int(O.dispatch(t.sv, A, "scan")[0][0])
        assert nxt < ENF
        t.sv["current_load"][nxt] = t.sv["num_processors"][nxt]
        want = t.turn(A, upd_idx=[nxt], where=7)
        assert nxt not in want
        # 8: three servants picked earlier get a slot back
        rel = t.release(rng, 3)
        t.turn(A, rel=rel, where=8)
        t.turn(_rpc(0), rel=t.release(rng, 5), where=9)  # an empty call that only releases
        t.turn(A, where=10)
        t.checkpoint()
        assert t.mailbox == 9
    finally:
        t.close()


@pytest.mark.parametrize("seed,S", list(enumerate([300, 700, 1500, 3000, 6000, 12000])))
def test_resident_state_random(seed, S, key_mode):
    """150 turns: 0 .. 64 requests (identical with probability 0.7), 0 .. 16 heartbeat rows that
    change no structure, 0 .. 64 released grants; get_running every 25th turn."""
    sv = _pool(S, seed=600 + seed)
    t = Turns(sv, key_mode)
    rng = np.random.default_rng(7000 + seed)
    try:
        for turn in range(150):
            sv = t.sv
            idx = np.sort(rng.choice(S, size=int(rng.integers(0, 17)), replace=False))
            for s in idx:
                sv["current_load"][s] = rng.integers(0, int(sv["num_processors"][s]) + 3)
                if rng.random() < 0.2:
                    sv["memory_available"][s] = rng.integers(1 * GIB, 40 * GIB)
                if rng.random() < 0.1:  # capacity figures that keep min(max_tasks, nproc)
                    keep = min(int(sv["max_tasks"][s]), int(sv["num_processors"][s]))
                    if int(sv["max_tasks"][s]) == keep and keep:
                        sv["num_processors"][s] = keep + int(rng.integers(0, 9))
            rel = t.release(rng, int(rng.integers(0, 65)))
            n = int(rng.choice([0, 1, 2, 3, 4, 7, 8, 33, 63, 64]))
            tk = synth.make_tasks(n, sv, n_envs=3, seed=int(rng.integers(1 << 30)), self_frac=0.1)
            if n and rng.random() < 0.7:
                tk = {k: np.full(n, v[0], np.uint32) for k, v in tk.items()}
            t.turn(tk, upd_idx=idx, rel=rel, where=turn)
            if turn % 25 == 24:
                t.checkpoint(turn)
        t.checkpoint()
        assert t.mailbox > 60, (t.mailbox, t.commands)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------
# 6. The mailbox at its edges
# ---------------------------------------------------------------------------------------------
N_REL = [0, 1, 3, 4, 5, 6, 7, 8, 9, 63, 64]
N_UPD = [0, 1, 2, 15, 16]
N_TASKS = [0, 1, 2, 7, 8, 9, 64]


@pytest.mark.parametrize("packed,want_util", [("1", False), ("0", False), ("1", True), ("0", True)],
                         ids=["packed", "fp64", "packed-util", "fp64-util"])
def test_mailbox_edges_on_a_saturated_pool(packed, want_util, monkeypatch):
    """48 servants, 2 slots each, all taken: what a turn grants is what it releases or what a
    heartbeat row frees (a row can also close a servant that was just released), so a stale or
    missing payload word changes that turn's answer — or the answer of the drain that follows
    every turn (64 identical requests, a head-only command right behind one that used the arrays)
    until nothing is free. One resident life over the release counts around the head's 4 + 3 words
    and the array, the row counts around the head's single row, and request counts around the
    reply's 7 placements; then 65 releases / 17 rows, which a launched kernel takes through
    pointers."""
    monkeypatch.setenv("YDC_PACKED_TICK", packed)
    monkeypatch.setenv("YDC_RESIDENT_IDLE_MS", "20000")
    S = 48
    sv = _flat_pool(S, nproc=16, max_tasks=2, running=2)
    t = Turns(sv, packed == "1", want_util)
    t.held = [s for s in range(S) for _ in range(2)]
    rng = np.random.default_rng(48)
    closed = set()  # servants a heartbeat row keeps from being free (load, or low memory)

    def rows_for(n_upd, released):
        """Rows on n_upd servants: those that are closed open again, those released this turn are
        closed, the rest gets new figures that change nothing."""
        sv = t.sv
        idx = list(closed)[:n_upd]
        for s in idx:
            sv["current_load"][s] = int(rng.integers(0, 3))
            sv["memory_available"][s] = 32 * GIB
            closed.discard(s)
        for s in dict.fromkeys(released):
            if len(idx) == n_upd:
                break
            if s not in idx:
                if rng.random() < 0.5:
                    sv["current_load"][s] = 16 + 2 + int(rng.integers(0, 6))
                else:
                    sv["memory_available"][s] = 1 * GIB
                closed.add(s)
                idx.append(s)
        others = [int(s) for s in rng.permutation(S) if s not in idx and s not in closed]
        for s in others[:n_upd - len(idx)]:
            sv["num_processors"][s] = 16 + int(rng.integers(0, 9))
            sv["current_load"][s] = int(rng.integers(0, 3))
            idx.append(s)
        assert len(idx) == n_upd
        return np.sort(np.array(idx, np.uint32))

    def drain(where):
        for k in range(4):
            want = t.turn(_rpc(64, minv=20 * (k & 1), rip=FOREIGN + k), where=(where, "drain", k))
            if (want == TIMEOUT).any():
                return
        raise AssertionError("the pool does not saturate")

    try:
        drain("start")  # (launches the kernel of this life; everything after it is a mailbox command)
        first = t.commands
        for i in range(110):
            n_rel, n_upd, n = N_REL[i % 11], N_UPD[i % 5], N_TASKS[i % 7]
            assert len(t.held) >= n_rel
            rel = t.release(rng, n_rel)
            idx = rows_for(n_upd, rel)
            if (i // 7) % 2:
                tk = _rpc(n, minv=20 * (i & 1), rip=FOREIGN + i)
            else:  # distinct: other hosts (a servant's own among them), both version thresholds
                rip = FOREIGN + 100 + rng.permutation(64)[:n]
                if n > 2:
                    rip[1] = t.sv["ip"][int(rng.integers(S))]
                tk = {"env_id": np.zeros(n, np.uint32), "min_version": (20 * (np.arange(n) & 1)).astype(np.uint32),
                      "requestor_ip": rip.astype(np.uint32)}
            t.turn(tk, upd_idx=idx, rel=rel, where=(i, n_rel, n_upd, n))
            drain(i)
        assert t.mailbox == t.commands - first
        assert t.c.stats()["tick_launched_calls"] == 1
        # everything open again, then lists beyond the mailbox: a launched kernel, through pointers
        idx = rows_for(len(closed), [])
        t.turn(_rpc(0), upd_idx=idx, where="open all")
        drain("open all")
        assert len(t.held) == 96 and not closed
        launched, resident = t.launched, t.resident
        want = t.turn(_rpc(20), rel=t.release(rng, 65), where="65 releases")
        assert (want < ENF).all()
        assert (t.launched, t.resident) == (launched + 1, resident) and not t.alive
        drain("after 65 releases")  # (launches the next life)
        t.turn(_rpc(3), rel=t.release(rng, 9), where="second life")
        launched, resident = t.launched, t.resident
        rel = t.release(rng, 12)
        idx = rows_for(17, rel)
        t.turn(synth.make_tasks(9, t.sv, n_envs=1, seed=4, self_frac=0.0), upd_idx=idx, rel=rel, where="17 rows")
        assert (t.launched, t.resident) == (launched + 1, resident) and not t.alive
        drain("after 17 rows")
        t.checkpoint()
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------
# 7. A witness that the merge ran
# ---------------------------------------------------------------------------------------------
def _witness_calls(S):
    """name -> (pool, requests): one representative call of items 1 - 4."""
    sv = _pool(S, seed=100 + S)
    own, a, _ = _own_host_pool(S, "one")
    return {
        "rpc": (sv, _rpc(3, minv=20)),
        "dry": (_dry_list_pool(S)[0], _rpc(40)),
        "own_host": (own, _rpc(12, minv=20, rip=int(own["ip"][a]))),
        "two": (sv, _rpc(2, minv=20)),
        "distinct": (sv, synth.make_tasks(9, sv, n_envs=3, seed=S, self_frac=0.0)),
    }


def _witness_child():
    """Runs in a process of its own on the measurement build (YDC_LIB), every call a launch
    (YDC_RESIDENT=0: the kernel has ended when its stamps are read). Prints the stamps 27 .. 31."""
    import ctypes as C
    L = binding.lib()
    L.ydc_debug_phase_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    L.ydc_debug_phase_probe.restype = C.c_int
    out = {}
    for S in (900, 12000):
        for name, (sv, tk) in _witness_calls(S).items():
            c = binding.Context(device=0)
            c.upload_servants(pack.to_abi_columns(sv))
            want, _, wrun = O.dispatch(sv, tk, "scan")
            assert L.ydc_debug_phase_probe(None, 0, 1) == 0
            got, _ = c.dispatch_tick(tk)
            st = c.stats()
            assert st["small_batch"] == 1 and st["tick_resident_calls"] == 0, st
            buf = np.zeros(32, np.uint64)
            assert L.ydc_debug_phase_probe(buf.ctypes.data, buf.size, 0) == 0
            assert np.array_equal(got, want), (S, name, got, want)
            assert np.array_equal(c.get_running(), wrun), (S, name)
            c.close()
            out["%d/%s" % (S, name)] = {"words": [int(w) for w in buf[27:32]], "want": [int(w) for w in want]}
    print("WITNESS " + json.dumps(out))


def test_witness_that_the_merge_ran():
    """The measurement build stamps the merge: words 27 - 29 its first round's clock, word 30
    round + 1, word 31 the requests placed in round 0. At K = 4 and at 12000 servants with
    one-word candidates: an RPC of 3 is one round; the dry-list pool takes several rounds and
    places fewer than n in the first; a request from a host with an eligible free servant enters
    the merge and abandons it (no round counted); 2 requests and distinct requests never enter."""
    subprocess.check_call(["make", "-s", "probe"], cwd=ROOT)
    env = dict(os.environ, YDC_LIB=os.path.join(ROOT, "yadcc_amd", "libydc_probe.so"), YDC_RESIDENT="0",
               YDC_PACKED_TICK="1")
    env.pop("YDC_TUNE", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "witness"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("WITNESS ")][-1]
    out = json.loads(line[len("WITNESS "):])
    for S in (900, 12000):
        T = _threads(S)
        w = {name: out["%d/%s" % (S, name)] for name in ("rpc", "dry", "own_host", "two", "distinct")}
        # (the pool still gives the call its shape: no thread's two-entry list is used up before
        # the last pick, so one round places all three)
        assert len({x % T for x in w["rpc"]["want"][:-1]}) == 2 and max(w["rpc"]["want"]) < ENF
        w27, _, _, w30, w31 = w["rpc"]["words"]
        assert w27 != 0 and w30 == 1 and w31 == 3, (S, w["rpc"])
        w27, _, _, w30, w31 = w["dry"]["words"]
        assert w27 != 0 and w30 >= 2 and 0 < w31 < 40, (S, w["dry"])
        w27, _, _, w30, w31 = w["own_host"]["words"]
        assert w27 != 0 and w30 == 0, (S, w["own_host"])
        assert w["two"]["words"][0] == 0 and w["two"]["words"][3] == 0, (S, w["two"])
        assert w["distinct"]["words"][0] == 0 and w["distinct"]["words"][3] == 0, (S, w["distinct"])


if __name__ == "__main__":
    if sys.argv[1:] == ["witness"]:
        _witness_child()
