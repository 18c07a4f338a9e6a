"""Both builds of k_bin_sort (yadcc_amd/csrc/bin_sort.h: workgroups of 512 and of 1024 threads;
occupancy_plan.h picks one, YDC_BIN_THREADS forces either) against the oracle, with every bin sort
checked against a host sort of the staged records (YDC_BINSORT_VERIFY) and ydc_stats::radix_passes
== 0 (the bin sort placed the slots, no fallback).

A narrow workgroup orders the same bins in more rounds per thread, reads its run table in a loop and
keeps only ranks in registers across the counting passes' barriers, so the sizes here sit at the
edges of a wave (64), of a round (512, 1024) and of a bin's capacity (4096): pools of identical
servants, where every key occurs once per servant and one bin holds exactly n records."""
import functools
import os

import numpy as np
import pytest

from oracle import oraclebind as O
from tests import cases, class_edge_cases as K
from tests.test_gpu_parity import check
from yadcc_amd import binding, pack, streaming, synth

pytestmark = pytest.mark.gpu

WIDTHS = (512, 1024)
SIZES = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096)  # <= 4096: the bin sort's servant limit
CLASS_COUNTS = (1, 2, 5, 65, 66, 67, 68, 69, 70)
COLS = ("env_id", "min_version", "requestor_ip")
N_ENVS = 7  # digests of the class pools: masks 1 .. 35 fit 6 bits, the 7th is never offered


def _context(width, verify=True):
    """A context with the given k_bin_sort build forced. The switches are read at ydc_create."""
    want = {"YDC_BINSORT": "1", "YDC_BINSORT_VERIFY": "1" if verify else "0", "YDC_BIN_THREADS": str(width)}
    old = {k: os.environ.get(k) for k in want}
    os.environ.update(want)
    try:
        return binding.Context(device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", params=WIDTHS, ids=["threads%d" % w for w in WIDTHS])
def ctx(request):
    c = _context(request.param)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def tied_pool(n, n_classes, busy=False):
    """n identical servants (the shape of tests/test_binsort_gpu.py's _tied_pool) in n_classes classes:
    class c = i % n_classes of servant i has version 19 + (c & 1) and digest set (c >> 1) + 1, so the
    classes differ by version, by environment set, or both; the keys do not depend on either. busy:
    the servants already run 0 .. 7 tasks, so the bins start at ranks that are no multiple of 64.
    -> (servants, requests, classes the pool really has)."""
    sv = synth.make_servants(n, n_tasks_hint=4 * n, n_envs=1, seed=3)
    sv["version"][:] = 20
    sv["num_processors"][:] = 16
    sv["max_tasks"][:] = 8
    sv["current_load"][:] = 0
    sv["running_tasks"][:] = 0
    sv["priority"][:] = 2
    sv["total_memory"][:] = 64 << 30
    sv["memory_available"][:] = 32 << 30
    if n_classes > 1:
        cls = np.arange(n) % n_classes
        sv["version"][:] = (19 + (cls & 1)).astype(np.uint32)
        sv["env_mask"] = ((cls >> 1) + 1).astype(np.uint64)
    if busy:
        sv["running_tasks"][:] = (np.arange(n) * 7 % 8).astype(np.uint32)
    n_envs = 1 if n_classes == 1 else N_ENVS
    tk = synth.make_tasks(max(64, 3 * n), sv, n_envs=n_envs, seed=5 + n, self_frac=0.1)
    return sv, tk, K.plan_of(sv, len(tk["env_id"]))["C"]


@pytest.mark.parametrize("n_classes", CLASS_COUNTS)
def test_single_bin_ties_at_wave_round_and_capacity_edges(ctx, n_classes):
    """Every size with 1 class (single-bin ties), and the same pools with 2, 5 and 65 .. 70 classes:
    the class partition and the level table across 1 .. 8 / 1 .. 16 waves and, beyond 64 classes,
    class bits past one ballot word."""
    for n in SIZES:
        sv, tk, C = tied_pool(n, n_classes)
        assert C == min(n, n_classes), (n, n_classes, C)
        st = check(ctx, sv, tk)
        assert st["radix_passes"] == 0 and st["n_classes"] == C, (n, n_classes, st)
        assert st["n_slots"] == 8 * n, (n, st)


@pytest.mark.parametrize("n_classes", (1, 2, 5, 66))
def test_busy_servants_skew_the_level_table(ctx, n_classes):
    """Servants that already run tasks: fewer slots each, bins that start mid-wave (the walk of the
    places is aligned to the global rank, not to the bin)."""
    for n in (65, 513, 1025, 4096):
        sv, tk, C = tied_pool(n, n_classes, busy=True)
        st = check(ctx, sv, tk)
        assert st["radix_passes"] == 0 and st["n_classes"] == C, (n, n_classes, st)
        assert st["n_slots"] == int((8 - sv["running_tasks"].astype(np.int64)).sum()), (n, st)


def test_busy_random_pool(ctx):
    sv, tk = cases.random_case(seed=81, n_tasks=20_000, n_servants=1500, n_envs=4, self_frac=0.2,
                               initial_running=True)
    st = check(ctx, sv, tk)
    assert st["radix_passes"] == 0


@functools.lru_cache(maxsize=None)
def seeded_case():
    sv, tk = cases.random_case(seed=91, n_tasks=20_000, n_servants=1500, n_envs=3, unknown_env_frac=0.002,
                               self_frac=0.15)
    return sv, tk, O.dispatch(sv, tk, "sorted")


def test_both_widths_agree():
    """One seeded case of 20k requests x 1500 servants: servant_idx and running_tasks of the two
    builds are equal array for array (and the oracle's)."""
    sv, tk, (want, _, wrun) = seeded_case()
    got = {}
    for width in WIDTHS:
        c = _context(width)
        try:
            c.upload_servants(pack.to_abi_columns(sv))
            idx, _, run = c.dispatch(tk)
            st = c.stats()
            assert st["radix_passes"] == 0, (width, st)
            got[width] = (idx, run)
        finally:
            c.close()
    assert np.array_equal(got[512][0], got[1024][0]) and np.array_equal(got[512][1], got[1024][1])
    assert np.array_equal(got[512][0], want) and np.array_equal(got[512][1], wrun)


@pytest.mark.parametrize("width", WIDTHS)
def test_streaming_ticks_take_the_forced_width(width):
    """The captured step of a stream launches whichever build its plan names: four ticks of 1000
    requests on 1500 servants, each equal to the oracle on the registry as the stream has it."""
    sv, _ = cases.random_case(seed=93, n_tasks=20_000, n_servants=1500, n_envs=2)
    es = streaming.EventStream(sv, 3000, 1000)
    c = _context(width)
    try:
        c.upload_servants(pack.to_abi_columns(sv))
        c.stream_begin(es.hb + 8, 1000, 3000)
        for t in range(4):
            who, rows, rel, tk = es.next_tick()
            want, _, wrun = O.dispatch(es.registry_snapshot(), tk, "sorted")
            got = c.stream_tick(who, rows, rel, tk)
            assert np.array_equal(got, want), t
            assert c.stats()["radix_passes"] == 0, t
            es.commit(got)
            assert np.array_equal(c.get_running(), wrun), t
        c.stream_end()
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def lanes_case():
    sv, tk_a = cases.random_case(seed=61, n_tasks=8000, n_servants=300, n_envs=3, self_frac=0.15,
                                 unknown_env_frac=0.01)
    tk_b = synth.make_tasks(8000, sv, n_envs=3, seed=977, unknown_env_frac=0.01, self_frac=0.15)
    return sv, (tk_a, tk_b)


@pytest.mark.parametrize("width", WIDTHS)
def test_two_lanes_at_a_small_size(width):
    """8k requests x 300 servants, 24 batches two deep with alternating request columns and result
    buffers of their own: every batch equals the synchronous result of the same context, batches
    went to the second lane, and none had to be placed again. (Without YDC_BINSORT_VERIFY: a
    verified bin sort is placed when waited for, on one lane.)"""
    sv, tks = lanes_case()
    DA = binding.DeviceArray
    c = _context(width, verify=False)
    try:
        c.upload_servants(pack.to_abi_columns(sv))
        cols = [[DA.from_numpy(tk[k]) for k in COLS] for tk in tks]
        sync = []
        for b in range(2):
            out = DA.from_numpy(np.full(8000, 0xDEADBEEF, np.uint32))
            run = DA.from_numpy(np.full(300, 0xDEADBEEF, np.uint32))
            c.dispatch_device(*cols[b], out, None, run)
            sync.append((out.numpy(), run.numpy()))
            assert c.stats()["radix_passes"] == 0
            want, _, wrun = O.dispatch(sv, tks[b], "sorted")
            assert np.array_equal(sync[b][0], want) and np.array_equal(sync[b][1], wrun), b
        n = 24
        outs = [DA.from_numpy(np.full(8000, 0xDEADBEEF, np.uint32)) for _ in range(n)]
        runs = [DA.from_numpy(np.full(300, 0xDEADBEEF, np.uint32)) for _ in range(n)]
        before = c.debug_pipeline()
        c.dispatch_device_async(*cols[0], outs[0], None, runs[0])
        for b in range(1, n):
            c.dispatch_device_async(*cols[b & 1], outs[b], None, runs[b])
            c.dispatch_wait()
        c.dispatch_wait()
        for b in range(n):
            assert np.array_equal(outs[b].numpy(), sync[b & 1][0]), b
            assert np.array_equal(runs[b].numpy(), sync[b & 1][1]), b
        batches, second, misses = (x - y for x, y in zip(c.debug_pipeline(), before))
        print("width %d: batches %d, on the second lane %d, misses %d" % (width, batches, second, misses))
        assert second >= 3 and misses == 0, (batches, second, misses)
    finally:
        c.close()
