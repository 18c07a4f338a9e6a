"""Pipelined batches on two device lanes (yadcc_amd/csrc/lane_rule.h; ydc_dispatch_device_async /
ydc_dispatch_wait): a batch that does not depend on the outstanding one is enqueued on the other
lane — another stream, another workspace, other DeviceParams — and runs beside it. Every placement
and every running_tasks column is the oracle's; the two batches of a test have different request
columns (3000 and 1900 requests: 47 and 30 chunks of 64, several hand-offs per launch), so a
mixed-up workspace is a wrong answer. Three plans: the bin sort, the radix sort, and a registry of
65 .. 128 classes (two mask words per request)."""
import functools

import numpy as np
import pytest

from oracle import oraclebind as O
from tests import cases, class_edge_cases as K
from tests.test_context_lifetime_gpu import rows_of
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu

COLS = ("env_id", "min_version", "requestor_ip")
N_A, N_B, N_SERVANTS = 3000, 1900, 300
# name -> (switches read at ydc_create, digests of the registry)
PLANS = {"binsort": ({}, 3), "radix": ({"YDC_BINSORT": "0"}, 3), "two_mask_words": ({}, 6)}


@functools.lru_cache(maxsize=None)
def case(n_envs):
    """The registry, the two batches and what the oracle places for either on the unchanged registry."""
    sv, tk_a = cases.random_case(seed=61, n_tasks=N_A, n_servants=N_SERVANTS, n_envs=n_envs, self_frac=0.15,
                                 unknown_env_frac=0.01)
    tk_b = synth.make_tasks(N_B, sv, n_envs=n_envs, seed=977, unknown_env_frac=0.01, self_frac=0.15)
    n_classes = K.plan_of(sv, N_A)["C"]
    assert (64 < n_classes <= 128) if n_envs == 6 else n_classes <= 64, n_classes
    want = [O.dispatch(sv, tk, "sorted") for tk in (tk_a, tk_b)]
    assert not np.array_equal(want[0][0][:N_B], want[1][0])
    return sv, (tk_a, tk_b), [(w[0], w[2]) for w in want]


def context(monkeypatch, plan, **more):
    env, n_envs = PLANS[plan]
    for k in ("YDC_BINSORT", "YDC_LANES", "YDC_HAND_TRIES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in {**env, **more}.items():
        monkeypatch.setenv(k, v)
    sv, tks, want = case(n_envs)
    c = binding.Context(device=0)
    c.upload_servants(pack.to_abi_columns(sv))
    return c, sv, tks, want


def device_columns(tks):
    return [[binding.DeviceArray.from_numpy(tk[k]) for k in COLS] for tk in tks]


def results(n_batches, sizes, n_servants):
    DA = binding.DeviceArray
    outs = [DA.from_numpy(np.full(sizes[b & 1], 0xDEADBEEF, np.uint32)) for b in range(n_batches)]
    runs = [DA.from_numpy(np.full(n_servants, 0xDEADBEEF, np.uint32)) for _ in range(n_batches)]
    return outs, runs


def run_two_deep(c, cols, outs, runs, commits=None):
    """Batch b from column set b & 1, two in flight."""
    n = len(outs)
    commits = commits or [False] * n
    c.dispatch_device_async(*cols[0], outs[0], None, runs[0], commit=commits[0])
    for b in range(1, n):
        c.dispatch_device_async(*cols[b & 1], outs[b], None, runs[b], commit=commits[b])
        c.dispatch_wait()
    c.dispatch_wait()


def eight_batches(c, sv, tks, want):
    cols = device_columns(tks)
    outs, runs = results(8, (N_A, N_B), len(sv["version"]))
    run_two_deep(c, cols, outs, runs)
    for b in range(8):
        idx, run = want[b & 1]
        got = outs[b].numpy()
        bad = np.nonzero(got != idx)[0]
        assert bad.size == 0, (b, bad[:5], got[bad[:5]], idx[bad[:5]])
        assert np.array_equal(runs[b].numpy(), run), b
    assert np.array_equal(c.get_running(), np.asarray(sv["running_tasks"], np.uint32))
    return c.debug_pipeline()


@pytest.mark.parametrize("plan", list(PLANS))
def test_two_lanes_bit_exact(monkeypatch, plan):
    """Eight no-COMMIT batches, alternately from the two column sets, each with its own out_idx and
    out_running: every one is the oracle's on the unchanged registry, the registry is untouched, and
    at least three of them went to the second lane."""
    c, sv, tks, want = context(monkeypatch, plan)
    batches, second, misses = eight_batches(c, sv, tks, want)
    print("batches %d, on the second lane %d, misses %d" % (batches, second, misses))
    assert second >= 3, (batches, second, misses)
    c.close()


@pytest.mark.parametrize("plan", list(PLANS))
def test_same_answers_with_lanes_off(monkeypatch, plan):
    c, sv, tks, want = context(monkeypatch, plan, YDC_LANES="0")
    batches, second, misses = eight_batches(c, sv, tks, want)
    assert second == 0, (batches, second, misses)
    c.close()


@pytest.mark.parametrize("plan", list(PLANS))
def test_mixed_commit(monkeypatch, plan):
    """no-COMMIT, COMMIT, no-COMMIT, no-COMMIT, COMMIT, no-COMMIT: the oracle applied in that order,
    only the COMMIT batches advancing the registry."""
    c, sv, tks, _ = context(monkeypatch, plan)
    commits = [False, True, False, False, True, False]
    reg = dict(sv)
    want = []
    for b, commit in enumerate(commits):
        idx, _, run = O.dispatch(reg, tks[b & 1], "sorted")
        want.append((idx, run))
        if commit:
            reg = dict(reg, running_tasks=run)
    cols = device_columns(tks)
    outs, runs = results(len(commits), (N_A, N_B), len(sv["version"]))
    run_two_deep(c, cols, outs, runs, commits)
    for b, (idx, run) in enumerate(want):
        assert np.array_equal(outs[b].numpy(), idx), b
        assert np.array_equal(runs[b].numpy(), run), b
    assert np.array_equal(c.get_running(), np.asarray(reg["running_tasks"], np.uint32))
    c.close()


@pytest.mark.parametrize("plan", list(PLANS))
def test_misses_are_replayed(monkeypatch, plan):
    """Hand-off patience 0: the batches are not final within their pre-launched passes and
    ydc_dispatch_wait places them again — same answers, and misses were counted."""
    c, sv, tks, want = context(monkeypatch, plan, YDC_HAND_TRIES="0")
    batches, second, misses = eight_batches(c, sv, tks, want)
    print("batches %d, on the second lane %d, misses %d" % (batches, second, misses))
    assert misses > 0, (batches, second, misses)
    c.close()


def test_aliased_outputs_do_not_overlap(monkeypatch):
    """Two outstanding no-COMMIT batches with the same out_idx stay on one lane, in order: the buffer
    ends up with the second batch's placement (and, behind it, the rest of the first's)."""
    c, sv, tks, want = context(monkeypatch, "binsort")
    cols = device_columns(tks)
    outs, runs = results(4, (N_A, N_B), len(sv["version"]))
    run_two_deep(c, cols, outs[:2], runs[:2])  # (the first batches after the upload: lane 0 settles)
    second0 = c.debug_pipeline()[1]
    shared = binding.DeviceArray.from_numpy(np.full(N_A, 0xDEADBEEF, np.uint32))
    c.dispatch_device_async(*cols[0], shared, None, runs[0])
    c.dispatch_device_async(*cols[1], shared, None, runs[1])
    c.dispatch_wait()
    c.dispatch_wait()
    got = shared.numpy()
    assert np.array_equal(got[:N_B], want[1][0]) and np.array_equal(got[N_B:], want[0][0][N_B:])
    assert c.debug_pipeline()[1] == second0
    # ... and the same pair with outputs of their own does overlap.
    c.dispatch_device_async(*cols[0], outs[2], None, runs[2])
    c.dispatch_device_async(*cols[1], outs[3], None, runs[3])
    c.dispatch_wait()
    c.dispatch_wait()
    assert np.array_equal(outs[2].numpy(), want[0][0]) and np.array_equal(outs[3].numpy(), want[1][0])
    assert c.debug_pipeline()[1] == second0 + 1
    c.close()


@pytest.mark.parametrize("joined_by_the_update", [False, True])
def test_registry_change_between_batches(monkeypatch, joined_by_the_update):
    """update_servants on 20 rows (another current_load) between two pairs of overlapped batches:
    the first pair sees the old registry, the second the new one — also when the update is called
    while the first pair is still outstanding (it joins both lanes)."""
    c, sv, tks, want = context(monkeypatch, "binsort")
    cols = device_columns(tks)
    outs, runs = results(6, (N_A, N_B), len(sv["version"]))
    run_two_deep(c, cols, outs[:2], runs[:2])  # (lane 0 settles)
    rng = np.random.default_rng(5)
    idx = np.sort(rng.choice(N_SERVANTS, 20, replace=False))
    sv2 = {k: np.array(v) for k, v in sv.items()}
    sv2["current_load"][idx] = (sv2["current_load"][idx] + 1 + rng.integers(0, 40, 20)).astype(np.uint32)
    want2 = [O.dispatch(sv2, tk, "sorted") for tk in tks]
    assert not np.array_equal(want2[0][0], want[0][0])
    second0 = c.debug_pipeline()[1]
    c.dispatch_device_async(*cols[0], outs[2], None, runs[2])
    c.dispatch_device_async(*cols[1], outs[3], None, runs[3])
    assert c.debug_pipeline()[1] == second0 + 1
    if not joined_by_the_update:
        c.dispatch_wait()
        c.dispatch_wait()
    c.update_servants(idx, rows_of(sv2, idx))
    if joined_by_the_update:
        c.dispatch_wait()
        c.dispatch_wait()
    for b in (2, 3):
        assert np.array_equal(outs[b].numpy(), want[b & 1][0]) and np.array_equal(runs[b].numpy(), want[b & 1][1]), b
    c.dispatch_device_async(*cols[0], outs[4], None, runs[4])
    c.dispatch_device_async(*cols[1], outs[5], None, runs[5])
    c.dispatch_wait()
    c.dispatch_wait()
    for b in (4, 5):
        assert np.array_equal(outs[b].numpy(), want2[b & 1][0]) and np.array_equal(runs[b].numpy(), want2[b & 1][2]), b
    c.close()


def test_close_with_a_batch_on_each_lane(monkeypatch):
    c, sv, tks, want = context(monkeypatch, "binsort")
    cols = device_columns(tks)
    outs, runs = results(4, (N_A, N_B), len(sv["version"]))
    run_two_deep(c, cols, outs[:2], runs[:2])  # (lane 0 settles)
    second0 = c.debug_pipeline()[1]
    c.dispatch_device_async(*cols[0], outs[2], None, runs[2])
    c.dispatch_device_async(*cols[1], outs[3], None, runs[3])
    assert c.debug_pipeline()[1] == second0 + 1
    c.close()
    fresh = binding.Context(device=0)
    fresh.upload_servants(pack.to_abi_columns(sv))
    out = binding.DeviceArray.from_numpy(np.full(N_A, 0xDEADBEEF, np.uint32))
    fresh.dispatch_device(*cols[0], out)
    assert np.array_equal(out.numpy(), want[0][0])
    fresh.close()
