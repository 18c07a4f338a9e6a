"""The sort key at its edges, on the device: the pools of tests/key_edge_cases.py (adjacent
fractions with denominators next to 2^cap_bits, equal fractions on several servants, growing
capacities, tier crossings, at every key width) through the batch pipeline — bin sort, radix
sort with and without the fused class pass —, the tick kernel on both sides of its switch between
the packed word and the double, and the key windows of the sharded path. Everything against the
oracle's literal restatement: equal placements, equal doubles, equal running_tasks."""
import numpy as np
import pytest

from oracle import oraclebind as O
from tests import key_edge_cases as K
from tests.test_gpu_parity import check
from yadcc_amd import binding, pack

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 5, 8, 9, 10, 11, 12, 15, 16, 17, 20, 21, 22, 27)
FEW_CLASSES = ("one", "three", "parts3", "shared")
GIB = 1 << 30


def pool(b, variant, order, near_zero):
    if b == K.FP64_BITS:
        return K.fp64_pool(variant, order)
    return K.edge_pool(b, variant, order, near_zero=near_zero)


def pools(b, variants=K.VARIANTS):
    for variant in variants:
        for order in (0, 1):
            for near_zero in (True, False) if b <= K.MAX_EXACT_BITS else (False,):
                yield variant, order, near_zero, pool(b, variant, order, near_zero)


def batches(b, sv, variant, near_zero):
    """Plain; pools without near-zero servants also with an unknown digest (and a Timeout tail:
    they are smaller than their batch)."""
    yield K.edge_tasks(sv, variant, seed=b)
    if not near_zero:
        yield K.edge_tasks(sv, variant, seed=b + 1, unknown=True, own_frac=0.0)


N_PARTS = {"parts3": 3, "parts17": 17}


@pytest.mark.parametrize("b", WIDTHS)
def test_batch_pipeline_as_planned(b, monkeypatch):
    """The plan's own choice (the bin sort wherever it applies, checked against a host sort by
    YDC_BINSORT_VERIFY): b <= 10 evaluates the bin boundaries with the 32-bit form, b == 11 with
    the 64-bit form — the only place the device runs it."""
    monkeypatch.setenv("YDC_BINSORT_VERIFY", "1")
    c = binding.Context(device=0)
    planned = set()
    try:
        for variant, order, near_zero, sv in pools(b):
            for tk in batches(b, sv, variant, near_zero):
                assert len(tk["env_id"]) > 64
                st = check(c, sv, tk, "scan")
                where = (b, variant, order, near_zero, st)
                assert st["key_bits"] == K.expected_key_bits(b, variant), where
                assert st["small_batch"] == 0, where
                # 0: the bin sort placed the slots — wherever the plan allows it, and never a quiet
                # retry with the radix sort behind an overflowing bin
                key_bits, passes, binsort = K.plan_formats(sv, st["n_classes"], N_PARTS.get(variant, 1))
                assert key_bits == st["key_bits"], where
                assert st["radix_passes"] == (0 if binsort else passes), (where, binsort, passes)
                planned.add((variant, binsort))
    finally:
        c.close()
    # b == 11 is the case that matters: every variant but the 17 parts (whose 27-bit keys leave a
    # bin's record no room in its word) is bin-sorted there, as at every width below
    want = {(v, b <= 11 and not (v == "parts17" and b >= 10)) for v in K.VARIANTS}
    assert planned == want, (b, sorted(planned))


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("b", WIDTHS)
def test_batch_pipeline_radix_sort(b, fused, monkeypatch):
    """YDC_BINSORT=0: 32-bit radix keys up to b == 15, 64-bit ones (33 .. 43 bits and the part id,
    4 .. 5 passes) up to 21, the double beyond; the class partition fused into the last pass and
    as a pass of its own."""
    monkeypatch.setenv("YDC_BINSORT", "0")
    monkeypatch.setenv("YDC_FUSED_CLASS", str(fused))
    c = binding.Context(device=0)
    try:
        for variant, order, near_zero, sv in pools(b, K.VARIANTS if fused else FEW_CLASSES):
            for tk in batches(b, sv, variant, near_zero):
                st = check(c, sv, tk, "scan")
                where = (b, variant, order, near_zero, st)
                assert st["key_bits"] == K.expected_key_bits(b, variant), where
                key_bits, passes, _ = K.plan_formats(sv, st["n_classes"], N_PARTS.get(variant, 1))
                assert (st["key_bits"], st["radix_passes"]) == (key_bits, passes), where
    finally:
        c.close()


@pytest.mark.parametrize("b", WIDTHS)
def test_batch_committed_in_two_halves_cut_inside_equal_keys(b):
    """Two committed batches == one: the cut falls between two requests that took slots of EQUAL
    utilisation in the same tier (the second half starts inside the group of equal keys)."""
    sv = pool(b, "three", 0, False)  # (without near-zero servants: the equal fractions get their turn)
    tk = K.edge_tasks(sv, "three", seed=40 + b, own_frac=0.0)
    want, wutil, wrun = O.dispatch(sv, tk, "scan")
    granted = want < O.IDX_ENV_NOT_FOUND
    run = sv["running_tasks"].astype(np.int64)
    tier = np.full(len(want), -1)
    for i in np.nonzero(granted)[0]:  # (the slot a grant took: the servant's running_tasks at that time)
        s = int(want[i])
        tier[i] = 0 if sv["priority"][s] == 1 and 2 * run[s] < sv["num_processors"][s] else 1
        run[s] += 1
    same = np.nonzero(granted[:-1] & granted[1:] & (wutil[:-1] == wutil[1:]) & (want[:-1] != want[1:]) &
                      (tier[:-1] == tier[1:]))[0]
    assert same.size, "no two consecutive grants of equal utilisation on different servants"
    cut = int(same[len(same) // 2]) + 1
    c = binding.Context(device=0)
    try:
        c.upload_servants(pack.to_abi_columns(sv))
        first, u1, _ = c.dispatch({k: v[:cut] for k, v in tk.items()}, commit=True)
        second, u2, run = c.dispatch({k: v[cut:] for k, v in tk.items()}, commit=True)
        got = np.concatenate([first, second])
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (b, cut, bad[:5], got[bad[:5]], want[bad[:5]])
        assert np.array_equal(np.concatenate([u1, u2]), wutil)
        assert np.array_equal(run, wrun) and np.array_equal(c.get_running(), wrun)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# The tick kernel: the packed word (key above the registry index) while
# 2 * cap_bits + 1 + idx_bits <= 32 and cap_bits <= 10, the double beyond.
# ---------------------------------------------------------------------------------------------
TICK_SIZES = [(10, 2048, True), (10, 2049, False), (9, 8192, True), (9, 8193, False), (8, 16384, True),
              (11, 300, False)]


def tick_pool(b, S, near_zero):
    """The 3-class edge pool, its first half at the lowest registry indices, its second half at
    the highest, servants without a free slot between them."""
    edge = K.edge_pool(b, "three", 0, near_zero=near_zero)
    E = len(edge["version"])
    pad = S - E
    fill = {"version": 20, "num_processors": 64, "current_load": 0, "max_tasks": 40, "running_tasks": 40,
            "priority": 2, "total_memory": 64 * GIB, "memory_available": 32 * GIB, "env_mask": 1, "ip": 0,
            "port": 8335}
    sv = {k: np.concatenate([v[:E // 2], np.full(pad, fill[k], v.dtype), v[E // 2:]]) for k, v in edge.items()}
    sv["ip"] = ((10 << 24) + 1 + np.arange(S)).astype(np.uint32)
    return sv


def tick_packed(b, S):
    idx_bits = 1
    while (1 << idx_bits) < max(S, 2):
        idx_bits += 1
    return b <= 10 and 2 * b + 1 + idx_bits <= 32


def tick_commands(sv, S, packed):
    """2 .. 64 identical requests (the merge) and 1 .. 64 distinct ones (the loop) — as many as
    the kernel takes at this registry size."""
    from tests.test_tick_merge_gpu import _rpc, _tick_limit
    same, loop = _tick_limit(S, True, packed), _tick_limit(S, False, packed)
    out = []
    for i, n in enumerate((2, 3, min(33, same), same)):
        out.append(_rpc(n, env=i & 1, minv=20 * (i >> 1 & 1), rip=K.FOREIGN + i))
    for i, n in enumerate((1, 9, loop)):
        out.append(K.edge_tasks(sv, "three", seed=90 + i, n=n, own_frac=0.2))
    out.append(_rpc(same, env=0, minv=0, rip=int(sv["ip"][0])))  # an RPC from an edge servant's host
    return out


@pytest.mark.parametrize("b,S,packed", TICK_SIZES, ids=["b%d-S%d" % (b, S) for b, S, _ in TICK_SIZES])
def test_tick_kernel_resident(b, S, packed, monkeypatch):
    from tests.test_tick_merge_gpu import Turns
    monkeypatch.setenv("YDC_RESIDENT_IDLE_MS", "20000")
    assert tick_packed(b, S) == packed
    if (b, S) == (10, 2048):
        assert 2 * b + 1 + 11 == 32  # the word is full: the tier bit is bit 31
    sv = tick_pool(b, S, near_zero=True)
    t = Turns(sv, packed)
    try:
        for i, tk in enumerate(tick_commands(sv, S, packed)):
            t.turn(tk, where=(b, S, i))
            assert t.c.stats()["small_batch"] == 1, (b, S, i)
        t.checkpoint((b, S))
        assert t.mailbox == t.commands - 1 and t.commands == 8
    finally:
        t.close()


@pytest.mark.parametrize("b,S,packed", TICK_SIZES, ids=["b%d-S%d" % (b, S) for b, S, _ in TICK_SIZES])
def test_tick_kernel_launched(b, S, packed, monkeypatch):
    """Every command a launch of its own (YDC_RESIDENT=0), on the pool without near-zero servants:
    the near-one slots are what the requests take."""
    monkeypatch.setenv("YDC_RESIDENT", "0")
    sv = tick_pool(b, S, near_zero=False)
    c = binding.Context(device=0)
    try:
        c.upload_servants(pack.to_abi_columns(sv))
        for i, tk in enumerate(tick_commands(sv, S, packed)):
            want, wutil, wrun = O.dispatch(sv, tk, "scan")
            got, gutil = c.dispatch_tick(tk, commit=True, want_util=True)
            st = c.stats()
            assert np.array_equal(got, want), (b, S, i, got, want, st)
            assert np.array_equal(gutil, wutil), (b, S, i)
            assert st["small_batch"] == 1 and st["tick_resident_calls"] == 0, (b, S, i, st)
            sv["running_tasks"] = wrun
        if S > 4096:
            # The candidate format the kernel chose, where a stat shows it: past 4096 servants 64
            # identical requests are the tick kernel's with the one-word candidate only.
            from tests.test_tick_merge_gpu import _rpc
            tk = _rpc(64, env=0, minv=0, rip=K.FOREIGN + 9)
            want, wutil, wrun = O.dispatch(sv, tk, "scan")
            got, _ = c.dispatch_tick(tk, commit=True)
            assert np.array_equal(got, want), (b, S, got, want)
            assert c.stats()["small_batch"] == int(packed), (b, S, c.stats())
            sv["running_tasks"] = wrun
        assert np.array_equal(c.get_running(), sv["running_tasks"])
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# Sharded key windows (k_key_count, k_window: first_slot_not_below per servant and threshold)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("b", [12, 16, 21])
def test_sharded_key_windows(b, G, monkeypatch):
    from tests.test_sharded_gpu import check_against_oracle, make_group, sharded_run
    for order in (0, 1):
        sv = K.edge_pool(b, "three", order)
        tk = K.edge_tasks(sv, "three", seed=60 + b + G)
        n = len(tk["env_id"])
        cuts = [0] + sorted(np.random.default_rng(b + G).integers(1, n, G - 1).tolist()) + [n]
        for shard_sort in ("1", "0") if (order == 0 and G == 2) else ("1",):
            monkeypatch.setenv("YDC_SHARD_SORT", shard_sort)
            ctxs = make_group(G, sv)
            try:
                res = sharded_run(ctxs, sv, tk, cuts)
                check_against_oracle(res, sv, tk, "scan")
                for r in res:
                    assert r[3]["key_bits"] == K.expected_key_bits(b, "three")
                    assert r[3]["shard_sort_batches"] == (1 if shard_sort == "1" else 0), (b, G, order, r[3])
            finally:
                [c.close() for c in ctxs]
