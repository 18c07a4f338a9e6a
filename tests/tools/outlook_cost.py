"""Cost of the outlook's two read calls at the cfg5 shape, in one process: an rpc stream on 2 000
servants with inspection on, 40 000 to 50 000 leases in L (ticks of 10 000 rows until there are at
least 40 000) and 8 000 blocked RPCs in W. Medians of
`--reps` calls (host call to host return, buffers allocated once) of
  - ydc_stream_outlook_get for 1, 150 and 1 024 queries,
  - ydc_stream_inspect_waiting,
  - ydc_stream_inspect_servants, the yardstick: one small kernel plus copies.
    python tests/tools/outlook_cost.py --reps 50
prints one JSON line. Under `rocprofv3 --kernel-trace --stats -- python tests/tools/outlook_cost.py`
the kernel table gives the four k_outlook_* kernels beside k_inspect_servants. Needs the GPU."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

RPCS, MAX_ROWS, MAX_WAITING, LEASES, BLOCKED = 4_000, 1 << 16, 20_000, 40_000, 8_000
NIMM, NPRE = np.array([1, 1, 2, 2], np.uint32), np.array([0, 1, 1, 2], np.uint32)  # 2.5 rows on average
E64, E32, Z1 = np.empty(0, np.uint64), np.empty(0, np.uint32), np.zeros(1, np.uint32)
I64 = E64.view(np.int64)
FAR = 1 << 40


def us(v):
    return round(float(np.median(v)) * 1e6, 1)


def timed(call, reps):
    cost = []
    for _ in range(reps + 3):
        t0 = time.perf_counter()
        rc = call()
        cost.append(time.perf_counter() - t0)
        assert rc == 0, rc
    return us(cost[3:])


def build(sv, abi):
    """-> the context: L filled by ticks nobody frees, then every servant reports a load that leaves it
    no slot, and the RPCs of two further ticks all wait."""
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    S = len(sv["version"])
    es = streaming.EventStream(sv, RPCS, 0)
    rng = np.random.default_rng(5)
    ctx.stream_begin_rpc(S + 8, 16, RPCS, MAX_ROWS, MAX_WAITING, 1 << 18, 16, 16, 16, 16)
    ctx.stream_inspect_begin()
    t = n_leases = n_waiting = 0
    busy = False
    while n_waiting < BLOCKED:
        who, rows, _, tk = es.next_tick()
        if n_leases >= LEASES and not busy:
            who = np.arange(S, dtype=np.uint32)
            rows = np.zeros(S, dtype=binding.ROW_DTYPE)
            for k in ("version", "num_processors", "max_tasks"):
                rows[k] = sv[k]
            rows["current_load"] = sv["num_processors"]  # (load >= nproc: no capacity, :308-311)
            rows["flags"], rows["ip_id"], rows["env_mask"] = abi["flags"], abi["ip_id"], abi["env_mask"]
            busy = True
        elif busy:
            who, rows = who[:0], rows[:0]
        ni, npf = rng.choice(NIMM, RPCS), rng.choice(NPRE, RPCS)
        dl = np.full(RPCS, FAR if busy else t, np.int64)
        r = ctx.stream_tick_rpc(who, rows, E32, E64, I64, E64, E32, Z1, E64, tk, ni, npf, np.full(RPCS, FAR, np.int64), dl,
                                np.arange(t * RPCS, (t + 1) * RPCS, dtype=np.uint64), t)
        n_leases, n_waiting = r["n_leases"], r["n_waiting"]
        t += 1
    return ctx, n_leases, n_waiting


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    ctx, n_leases, n_waiting = build(sv, abi)
    L, h, S = binding.lib(), ctx._h, len(sv["version"])
    res = {"reps": a.reps, "servants": S, "leases": n_leases, "waiting": n_waiting}
    n = C.c_uint32(0)
    rng = np.random.default_rng(7)
    for q in (1, 150, 1024):
        env, minv = rng.integers(0, 64, q).astype(np.uint32), rng.choice(np.array([0, 20], np.uint32), q)
        env[0], minv[0] = 0, 0
        out = np.zeros(q, binding.OUTLOOK_DTYPE)
        res["outlook_%d_us" % q] = timed(lambda: L.ydc_stream_outlook_get(h, env.ctypes.data, minv.ctypes.data, q, out.ctypes.data),
                                         a.reps)
        assert out["waiting"][0] == n_waiting and out["leases"][0] == n_leases and out["free_servants"][0] == 0, out[0]
    cols = [np.empty(MAX_WAITING, t) for t in (np.uint64, np.uint32, np.uint32, np.uint32, np.int64, np.int64, np.uint32,
                                               np.uint32)]
    res["inspect_waiting_us"] = timed(lambda: L.ydc_stream_inspect_waiting(h, *[c.ctypes.data for c in cols], MAX_WAITING,
                                                                           C.byref(n)), a.reps)
    assert n.value == n_waiting
    disc, ever, run, avail = np.empty(S, np.int64), np.empty(S, np.uint64), np.empty(S, np.uint32), np.empty(S, np.uint32)
    tot = binding.StreamTotals()
    res["inspect_servants_us"] = timed(lambda: L.ydc_stream_inspect_servants(h, disc.ctypes.data, ever.ctypes.data, run.ctypes.data,
                                                                             avail.ctypes.data, S, C.byref(n), C.byref(tot)), a.reps)
    ctx.stream_end()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
