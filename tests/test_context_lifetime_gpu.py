"""The context's lifetime and its batch entry points as a caller sees them (ydc_api.hip): what
ydc_destroy gives back, that a call staged through the context's arenas leaves nothing behind for
the next one, and that heartbeats reach the same registry by either route. One 70-servant registry
throughout; every placement against the oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import oraclebind as O
from tests import cases
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu

N_SERVANTS = 70
DA = binding.DeviceArray


def free_device_memory():
    """hipMemGetInfo's free bytes — the figure torch.cuda.mem_get_info() reports — asked of the HIP
    runtime the library itself is bound to (the GPU test process does not load torch's second one)."""
    free, total = C.c_size_t(), C.c_size_t()
    fn = binding.lib().hipMemGetInfo
    fn.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    assert fn(C.byref(free), C.byref(total)) == 0
    return free.value


def rows_of(sv, idx):
    idx = np.asarray(idx, np.int64)
    rows = np.zeros(len(idx), binding.ROW_DTYPE)
    for k, col in (("version", "version"), ("num_processors", "num_processors"), ("current_load", "current_load"),
                   ("max_tasks", "max_tasks"), ("ip_id", "ip")):
        rows[k] = np.asarray(sv[col])[idx]
    rows["flags"] = pack.servant_flags(sv)[idx]
    em = np.asarray(sv["env_mask"])
    rows["env_mask"] = em[idx] if em.ndim == 1 else em[idx, 0]
    return rows


def one_round(monkeypatch):
    """Create, use every path once, close."""
    sv, tk = cases.random_case(seed=3, n_tasks=200, n_servants=N_SERVANTS, n_envs=3, self_frac=0.3)
    cols = pack.to_abi_columns(sv)
    # The batch pipeline from pageable memory, whatever the batch's size.
    monkeypatch.setenv("YDC_SMALL_BATCH", "0")
    c = binding.Context(device=0)
    monkeypatch.delenv("YDC_SMALL_BATCH")
    c.upload_servants(cols)
    c.dispatch(tk)
    assert c.stats()["small_batch"] == 0
    c.close()
    # Everything else on one context with the threshold at its default.
    c = binding.Context(device=0)
    c.upload_servants(cols)
    c.dispatch(tk)
    d_cols = [DA.from_numpy(tk[k]) for k in ("env_id", "min_version", "requestor_ip")]
    d_idx = [DA.from_numpy(np.zeros(200, np.uint32)) for _ in range(2)]
    for k in range(2):
        c.dispatch_device_async(d_cols[0], d_cols[1], d_cols[2], d_idx[k], None, None, commit=True)
    for k in range(2):
        c.dispatch_wait()
    held = [int(s) for s in d_idx[0].numpy() if s < O.IDX_ENV_NOT_FOUND]
    assert len(held) >= 3
    # A scheduler's turn with a heartbeat and a release: the kernel it launches stays resident.
    few = {k: v[:3] for k, v in tk.items()}
    c.dispatch_tick(few, [3], rows_of(sv, [3]), held[:1], commit=True)
    assert c.stats()["small_batch"] == 1
    c.release_slots(held[1:3])
    c.remove_servants([0, N_SERVANTS - 1])
    left = {k: np.delete(v, [0, N_SERVANTS - 1], axis=0) for k, v in sv.items()}
    c.stream_begin(4, 4, 16)
    for turn in range(2):
        c.stream_tick([turn], rows_of(left, [turn]), [], {k: v[:8] for k, v in tk.items()})
    c.close()  # (with the stream open and the resident kernel's box allocated)
    for a in d_cols + d_idx:
        a.free()


def test_destroy_gives_back_what_the_context_took(monkeypatch):
    """Six rounds of create / every path once / close: free device memory after rounds 2 to 6 equals
    that after round 1 (which pays for what the runtime itself keeps: code objects, its queues).
    Measured on the MI355X at the commit before the context owned its allocations and at this one:
    the six figures of a run were equal to the byte on both, so the allowance is 0."""
    free = []
    for _ in range(6):
        one_round(monkeypatch)
        free.append(free_device_memory())
    print("free device memory after each round:", free)
    assert all(f == free[0] for f in free[1:]), [f - free[0] for f in free]


def test_a_staged_call_leaves_nothing_behind():
    """ydc_dispatch from pageable memory (staged both ways), ydc_dispatch_device on device copies of the
    same columns, ydc_dispatch from page-locked buffers — one context, no COMMIT: all three are the
    oracle's placement, utilisation and running_tasks, bit for bit."""
    sv, tk = cases.random_case(seed=4, n_tasks=200, n_servants=N_SERVANTS, n_envs=3, self_frac=0.3, initial_running=True)
    want, wutil, wrun = O.dispatch(sv, tk, "sorted")
    c = binding.Context(device=0)
    c.upload_servants(pack.to_abi_columns(sv))

    def same(what, idx, util, run):
        assert np.array_equal(idx, want), what
        assert np.array_equal(util, wutil), what
        assert np.array_equal(run, wrun), what

    same("pageable", *c.dispatch(tk))
    d_cols = [DA.from_numpy(tk[k]) for k in ("env_id", "min_version", "requestor_ip")]
    d_idx = DA.from_numpy(np.full(200, 0xDEADBEEF, np.uint32))
    d_util = DA.from_numpy(np.full(200, -7.0, np.float64))
    d_run = DA.from_numpy(np.full(N_SERVANTS, 0xDEADBEEF, np.uint32))
    c.dispatch_device(d_cols[0], d_cols[1], d_cols[2], d_idx, d_util, d_run)
    same("device", d_idx.numpy(), d_util.numpy(), d_run.numpy())
    pinned = {}
    for k in ("env_id", "min_version", "requestor_ip"):
        pinned[k] = binding.pinned_empty(200, np.uint32)
        pinned[k][:] = tk[k]
    same("page-locked", *c.dispatch(pinned, out_idx=binding.pinned_empty(200, np.uint32)))
    assert np.array_equal(c.get_running(), np.asarray(sv["running_tasks"], np.uint32))
    c.close()


def update_lists(sv, rng):
    """Twelve heartbeat lists on the snapshot `sv` (changed in place, the way the servants would report):
    [(servants, the one the list is about)]. Light rows throughout; a version change, a host change,
    max_tasks to 0 and back, a mask change in word 1 only, an append."""
    n = len(sv["version"])

    def light(k):
        idx = np.sort(rng.choice(n, size=k, replace=False))
        for s in idx:
            sv["current_load"][s] = rng.integers(0, int(sv["num_processors"][s]) + 3)
            sv["memory_available"][s] = rng.integers(1 << 30, 40 << 30)
        return [int(s) for s in idx]

    yield light(3), None
    sv["version"][5] = 19 if sv["version"][5] == 20 else 20
    yield [5], 5
    yield light(5), None
    sv["ip"][9] = (10 << 24) + 5000
    yield sorted(set(light(2) + [9])), 9
    busy = int(np.argmax(np.minimum(sv["max_tasks"], sv["num_processors"])))
    was = int(sv["max_tasks"][busy])
    sv["max_tasks"][busy] = 0
    yield [busy], busy
    yield sorted(set(light(3) + [busy])), busy
    sv["max_tasks"][busy] = was
    yield [busy], busy
    sv["env_mask"][20, 1] ^= np.uint64(1 << 7)  # digest 71
    yield [20], 20
    for k in sv:  # a new servant: a copy of servant 1 on a host of its own
        sv[k] = np.concatenate([sv[k], sv[k][1:2]], axis=0)
    sv["ip"][n] = (10 << 24) + 6000
    sv["running_tasks"][n] = 0
    yield [n], n
    yield sorted(set(light(2) + [n])), n
    keep = int(sv["max_tasks"][30])
    if keep and keep <= int(sv["num_processors"][30]):
        sv["num_processors"][30] += 4  # (the capacity bound min(max_tasks, nproc) stays: no structure changes)
    yield [30], 30
    sv["version"][40] = 19 if sv["version"][40] == 20 else 20
    yield sorted(set(light(3) + [40])), 40


def test_the_two_heartbeat_routes_agree():
    """The same twelve update lists on two contexts over a registry of two mask words: one takes
    ydc_update_servants_wide and then ydc_dispatch, the other ydc_dispatch_tick with the rows riding
    along (COMMIT, the small-batch threshold at its default). After every list the placement of five
    requests and running_tasks are equal between the two and equal to the oracle, replayed on its own
    snapshot as in tests/test_tick_gpu.py."""
    n_envs = 100
    sv, _ = cases.random_case(seed=6, n_tasks=400, n_servants=N_SERVANTS, n_envs=n_envs)
    sv = {k: np.array(v, copy=True) for k, v in sv.items()}
    assert np.asarray(sv["env_mask"]).shape == (N_SERVANTS, 2)
    by_update, by_tick = binding.Context(device=0), binding.Context(device=0)
    for c in (by_update, by_tick):
        c.upload_servants(pack.to_abi_columns(sv))
    rng = np.random.default_rng(12)
    turns = 0
    for idx, about in update_lists(sv, rng):
        rows, masks = rows_of(sv, idx), np.asarray(sv["env_mask"])[idx]
        tk = synth.make_tasks(5, sv, n_envs=n_envs, seed=int(rng.integers(1 << 30)), self_frac=0.2)
        if about is not None:  # two of the five ask for a digest the servant the list is about advertises
            word = 0 if sv["env_mask"][about, 0] else 1
            m = int(sv["env_mask"][about, word])
            if m:
                tk["env_id"][:2] = 64 * word + (m & -m).bit_length() - 1
        want, _, wrun = O.dispatch(sv, tk, "scan")
        by_update.update_servants(idx, rows, env_masks=masks)
        a, _, _ = by_update.dispatch(tk, commit=True, want_util=False, want_running=False)
        b, _ = by_tick.dispatch_tick(tk, idx, rows, env_masks=masks, commit=True)
        assert np.array_equal(a, b) and np.array_equal(a, want), (turns, idx, a, b, want)
        ra, rb = by_update.get_running(), by_tick.get_running()
        assert np.array_equal(ra, rb) and np.array_equal(ra, wrun), (turns, idx)
        sv["running_tasks"] = wrun
        turns += 1
    assert turns == 12
    by_update.close()
    by_tick.close()
