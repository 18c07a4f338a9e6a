"""A group's lifetime as a caller sees it (ydc_api.hip, ydc_group_*): what ydc_group_destroy gives
back, and that a context leaves one group and joins another — or none — with its registry, its
placement and its counters intact. Local groups on device 0 (ydc_group_init_local), one pool of 300
servants, 3 digests and 3000 requests; every placement against the oracle. (The mailbox's second
export is in tests/test_sharded_multiprocess_gpu.py: its ranks are processes.)"""
import gc

import numpy as np
import pytest

from oracle import oraclebind as O
from tests import cases
from tests.test_context_lifetime_gpu import free_device_memory
from tests.test_sharded_gpu import check_against_oracle, sharded_run
from yadcc_amd import binding, pack

pytestmark = pytest.mark.gpu
DA = binding.DeviceArray


@pytest.fixture(scope="module")
def pool():
    sv, tk = cases.random_case(seed=91, n_tasks=3000, n_servants=300, n_envs=3, self_frac=0.1)
    return sv, tk, O.dispatch(sv, tk, "sorted")


def contexts(n, sv):
    ctxs = [binding.Context(device=0) for _ in range(n)]
    cols = pack.to_abi_columns(sv)
    for c in ctxs:
        c.upload_servants(cols)
    return ctxs


def grouped_batch(ctxs, sv, tk, cuts):
    """group_init_local, one sharded batch against the oracle, group_destroy on every rank."""
    binding.group_init_local(ctxs)
    res = sharded_run(ctxs, sv, tk, cuts)
    check_against_oracle(res, sv, tk)
    for c in ctxs:
        c.group_destroy()
    return res


def free_now():
    gc.collect()  # (the ranks' device arrays go with their threads' frames)
    return free_device_memory()


def test_a_group_gives_back_what_it_took(pool):
    """Six rounds of two contexts / group / one sharded batch / group_destroy / close: free device
    memory after rounds 2 to 6 is equal to the byte. Then two contexts that stay open: group, batch
    (which sizes what the contexts themselves keep), destroy, measure — and once more: the second
    group has left nothing behind that the first had not. Both hold to the byte on the MI355X at the
    commit before the group's workspace became one record, and at this one."""
    sv, tk, _ = pool
    n = len(tk["env_id"])
    free = []
    for _ in range(6):
        ctxs = contexts(2, sv)
        grouped_batch(ctxs, sv, tk, [0, n // 3, n])
        for c in ctxs:
            c.close()
        free.append(free_now())
    print("free device memory after each round:", free)
    assert all(f == free[1] for f in free[2:]), [f - free[1] for f in free]
    ctxs = contexts(2, sv)
    grouped_batch(ctxs, sv, tk, [0, n // 3, n])
    first = free_now()
    grouped_batch(ctxs, sv, tk, [0, n // 3, n])
    second = free_now()
    print("free device memory after the first and the second group of open contexts:", first, second)
    assert first == second, second - first
    for c in ctxs:
        c.close()


def test_regrouping(pool, monkeypatch):
    """Three contexts as a group of 3, the first two of them as a group of 2 with other cuts, then
    context 0 on its own: the oracle's placement every time. The sharded-sort counters belong to the
    context, not to the group: they go on counting across the groups (the registry is too small for
    a window to miss: every window is the whole registry) and stay when the context is alone."""
    monkeypatch.setenv("YDC_GROUP_BINSORT", "0")  # (a registry this small is bin-sorted whole otherwise)
    sv, tk, (want, wutil, wrun) = pool
    n = len(tk["env_id"])
    ctxs = contexts(3, sv)
    res = grouped_batch(ctxs, sv, tk, [0, n // 4, n // 2, n])
    print("group of 3:", [(r[3]["shard_sort_batches"], r[3]["shard_sort_misses"]) for r in res])
    assert all((r[3]["shard_sort_batches"], r[3]["shard_sort_misses"]) == (1, 0) for r in res)
    assert all(c.group_transport() == binding.TRANSPORT_NONE for c in ctxs)
    res = grouped_batch(ctxs[:2], sv, tk, [0, 2 * n // 3, n])
    print("group of 2:", [(r[3]["shard_sort_batches"], r[3]["shard_sort_misses"]) for r in res])
    assert all((r[3]["shard_sort_batches"], r[3]["shard_sort_misses"]) == (2, 0) for r in res)
    c = ctxs[0]
    assert c.group_transport() == binding.TRANSPORT_NONE
    d = [DA.from_numpy(tk[k]) for k in ("env_id", "min_version", "requestor_ip")]
    d_idx, d_util, d_run = DA(n, np.uint32), DA(n, np.float64), DA(len(wrun), np.uint32)
    c.dispatch_device(d[0], d[1], d[2], d_idx, d_util, d_run)
    assert np.array_equal(d_idx.numpy(), want)
    assert np.array_equal(d_util.numpy(), wutil)
    assert np.array_equal(d_run.numpy(), wrun)
    st = c.stats()
    print("alone:", (st["shard_sort_batches"], st["shard_sort_misses"]))
    assert (st["shard_sort_batches"], st["shard_sort_misses"]) == (2, 0)
    assert c.group_transport() == binding.TRANSPORT_NONE
    for c in ctxs:
        c.close()
