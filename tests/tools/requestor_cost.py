"""What asking for the load per requestor costs: a leased stream with inspection on
that holds --leases leases of 1 000 requestors, uniformly mixed ("uniform") or with one requestor
holding 90 % of them ("hot"), and --queries requestors asked for. Per mix and per form of the
counting kernels (equal requestors combined inside the wave: combine = 1, the default; an atomic per
lease: combine = 0, what YDC_TUNE requestor_combine=0 selects) a context of its own; in each,
alternating, medians of --repeats after a warm-up:
  find       ydc_stream_requestor_find: the table cleared, k_requestor_leases, k_requestor_find, the
             rows copied back;
  get        ydc_stream_requestor_get: the same build, k_requestor_fold, the rows copied back;
  host       what a scheduler has without the calls: ydc_stream_inspect_tasks +
             ydc_stream_inspect_waiting (host_get), then a numpy fold by requestor and the queries
             asked of it (host_fold, which includes host_get).
    python tests/tools/requestor_cost.py --leases 100000
prints one JSON line per context, times in microseconds of wall time from host call to host return
(every call ends in a device synchronise). Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, synth  # noqa: E402

E32, E64, I64 = np.empty(0, np.uint32), np.empty(0, np.uint64), np.empty(0, np.int64)
NO_ROWS = np.empty(0, binding.ROW_DTYPE)
SERVANTS, SLOTS, PER_TICK, REQUESTORS = 2048, 640, 50_000, 1000


def registry():
    sv = synth.make_servants(SERVANTS, n_tasks_hint=64, n_envs=1, seed=1)
    sv["version"][:], sv["num_processors"][:], sv["current_load"][:] = 20, SLOTS, 0
    sv["max_tasks"][:], sv["running_tasks"][:] = SLOTS, 0
    sv["memory_available"][:], sv["total_memory"][:] = 32 << 30, 64 << 30
    sv["env_mask"] = np.ones(SERVANTS, np.uint64)
    return sv


def requestors(mix, n, rng):
    ids = ((10 << 24) + 1 + np.arange(REQUESTORS)).astype(np.uint32)
    if mix == "uniform":
        return ids, rng.choice(ids, n)
    who = rng.choice(ids[1:], n)
    who[rng.random(n) < 0.9] = ids[0]
    return ids, who


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def host_fold(tasks, waiting, q):
    known = tasks["started_at"] != binding.INSPECT_NO_TIME
    ip = np.concatenate([tasks["requestor_ip"][known], waiting["requestor_ip"]])
    keys, at = np.unique(ip, return_inverse=True)
    nl = int(known.sum())
    leases = np.bincount(at[:nl], minlength=len(keys))
    zombies = np.bincount(at[:nl], weights=tasks["zombie"][known], minlength=len(keys))
    prefetch = np.bincount(at[:nl], weights=tasks["prefetch"][known], minlength=len(keys))
    waits = np.bincount(at[nl:], minlength=len(keys))
    rows = np.bincount(at[nl:], weights=waiting["n_immediate"].astype(np.int64) + waiting["n_prefetch"], minlength=len(keys))
    k = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    hit = keys[k] == q
    return hit, leases[k], zombies[k], prefetch[k], waits[k], rows[k]


def measure(leases, mix, combine, queries, repeats):
    os.environ["YDC_REQUESTOR_COMBINE"] = str(combine)
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(registry()))
    ctx.stream_begin_leased(8, 8, PER_TICK, leases + PER_TICK, 8, 8, 8, 8)
    ctx.stream_inspect_begin()
    rng = np.random.default_rng(5)
    ids, who = requestors(mix, leases, rng)
    now = 0
    for at in range(0, leases, PER_TICK):
        now += 1
        ip = who[at:at + PER_TICK]
        tk = {"env_id": np.zeros(len(ip), np.uint32), "min_version": np.zeros(len(ip), np.uint32), "requestor_ip": ip}
        out, _, _, _, n_leases = ctx.stream_tick_leased(E32, NO_ROWS, E32, E64, I64, E64, E32, np.zeros(1, np.uint32), E64, tk,
                                                        np.full(len(ip), 1 << 40, np.int64), now)
        assert (out < SERVANTS).all()
    assert n_leases == leases
    q = rng.choice(ids, queries).astype(np.uint32)
    q[: queries // 10] += np.uint32(1 << 20)  # (a tenth of the queries hold nothing)
    want = np.bincount(who - ids[0], minlength=REQUESTORS)
    T = {k: [] for k in ("find", "get", "host_get", "host_fold")}
    for r in range(repeats + 3):
        dt, (rows, un) = timed(lambda: ctx.stream_requestor_find(q))
        T["find"].append(dt)
        dt, (every, _) = timed(ctx.stream_requestors)
        T["get"].append(dt)
        assert un == 0 and np.array_equal(every["leases"], want[want > 0])
        dt_get, (tasks, waiting) = timed(lambda: (ctx.stream_inspect_tasks(), ctx.stream_waiting()))
        T["host_get"].append(dt_get)
        dt, (hit, l, z, p, w, wr) = timed(lambda: host_fold(tasks, waiting, q))
        T["host_fold"].append(dt_get + dt)
        assert np.array_equal(np.where(hit, l, 0), rows["leases"]) and not rows["waiting"].any()
    med = lambda x: round(float(np.median(x[3:])) * 1e6, 1)
    lo_hi = lambda x: [round(float(min(x[3:])) * 1e6, 1), round(float(max(x[3:])) * 1e6, 1)]
    res = {"leases": leases, "mix": mix, "combine": combine, "queries": queries, "repeats": repeats,
           "largest_share": round(float(want.max()) / leases, 3)}
    res.update({k + "_us": med(v) for k, v in T.items()})
    res.update(find_min_max_us=lo_hi(T["find"]))
    print(json.dumps(res), flush=True)
    ctx.stream_end()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leases", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    assert a.leases % PER_TICK == 0 and a.leases + PER_TICK <= SERVANTS * SLOTS
    for mix in ("uniform", "hot"):
        for combine in (1, 0):
            measure(a.leases, mix, combine, a.queries, a.repeats)


if __name__ == "__main__":
    main()
