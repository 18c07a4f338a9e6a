"""Cost of inspection (ydc_stream_inspect_begin) at the cfg5 shape, same process and same build:
  - a leased tick (10k requests, every grant of the previous tick freed by id, 200 heartbeats) and an
    rpc tick (4 000 RPCs, 10k rows) with inspection off and on: median wall time per tick (host call
    to host return);
  - the two get calls (ydc_stream_inspect_servants, ydc_stream_inspect_tasks) and, for comparison,
    ydc_stream_leases_get, with about 3 * 10^4 and 10^6 leases in the table.
    python tests/tools/inspect_tick_cost.py --ticks 300
prints one JSON line. Under `rocprofv3 --kernel-trace --stats -- python tests/tools/inspect_tick_cost.py
...` the kernel table gives k_lease_grant against k_lease_grant_inspect, k_rpc_grant against
k_rpc_grant_inspect, k_inspect_pack and k_inspect_servants. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

N, RPCS, MAX_ROWS, MAX_WAITING = 10_000, 4_000, 1 << 16, 20_000
NIMM, NPRE = np.array([1, 1, 2, 2], np.uint32), np.array([0, 1, 1, 2], np.uint32)  # 2.5 rows on average
E64, E32, Z1 = np.empty(0, np.uint64), np.empty(0, np.uint32), np.zeros(1, np.uint32)
I64 = E64.view(np.int64)
FAR = 1 << 40


def us(v):
    return round(float(np.median(v)) * 1e6, 1)


def leased_leg(sv, abi, ticks, inspect, ballast=0):
    """-> (tick times, the context with the stream still open)."""
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, 0)
    ctx.stream_begin_leased(es.hb + 8, N, N, ballast + 4 * N, 16, N, 16, 16)
    if inspect:
        ctx.stream_inspect_begin()
    held = 0
    while held < ballast:  # leases nobody frees; their slots go back by servant index
        who, rows, _, tk = es.next_tick()
        out, _, _, _, held = ctx.stream_tick_leased(who, rows, E32, E64, I64, E64, E32, Z1, E64, tk,
                                                    np.full(N, FAR, np.int64), 0)
        g = out[out < binding.IDX_ENV_NOT_FOUND]
        ctx.stream_tick_leased(E32, rows[:0], g, E64, I64, E64, E32, Z1, E64, {k: v[:0] for k, v in tk.items()}, I64, 0)
    live, cost = E64, []
    for t in range(ticks + 20):
        who, rows, _, tk = es.next_tick()
        lex = np.full(N, t + 6, np.int64)
        t0 = time.perf_counter()
        out, ids, _, _, _ = ctx.stream_tick_leased(who, rows, E32, E64, I64, live, E32, Z1, E64, tk, lex, t + 1)
        cost.append(time.perf_counter() - t0)
        g = out < binding.IDX_ENV_NOT_FOUND
        live = ids[g]
        es.commit(out)
        np.subtract.at(es.running, out[g], 1)  # (every grant is freed by id in the next tick)
        es.live = es.live[:0]
    return cost[20:], ctx


def rpc_leg(sv, abi, ticks, inspect):
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, RPCS, 0)
    rng = np.random.default_rng(5)
    ctx.stream_begin_rpc(es.hb + 8, 16, RPCS, MAX_ROWS, MAX_WAITING, 1 << 18, 16, MAX_ROWS, 16, 16)
    if inspect:
        ctx.stream_inspect_begin()
    live, cost = E64, []
    for t in range(ticks + 20):
        who, rows, _, tk = es.next_tick()
        ni, npf = rng.choice(NIMM, RPCS), rng.choice(NPRE, RPCS)
        tags = np.arange(RPCS, dtype=np.uint64)
        lease_for, dl = np.full(RPCS, 5, np.int64), np.full(RPCS, t, np.int64)  # (nothing waits)
        t0 = time.perf_counter()
        r = ctx.stream_tick_rpc(who, rows, E32, E64, I64, live, E32, Z1, E64, tk, ni, npf, lease_for, dl, tags, t)
        cost.append(time.perf_counter() - t0)
        g = np.repeat(np.arange(RPCS), ni + npf)
        ok = (np.arange(len(g)) - r["row_off"][g]) < r["n_granted"][g]
        live, srv = r["task_ids"][ok], r["servants"][ok]
        es.commit(srv)
        np.subtract.at(es.running, srv, 1)
        es.live = es.live[:0]
    ctx.stream_end()
    ctx.close()
    return cost[20:]


def get_calls(ctx, reps=7):
    out = {}
    for name, call in (("inspect_servants_us", ctx.stream_inspect_servants), ("inspect_tasks_us", ctx.stream_inspect_tasks),
                       ("leases_get_us", ctx.stream_leases)):
        cost = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = call()
            cost.append(time.perf_counter() - t0)
        out[name] = us(cost)
    out["leases"] = int(len(r[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--big", type=int, default=1_000_000)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    res = {"ticks": a.ticks}
    off, ctx = leased_leg(sv, abi, a.ticks, False, ballast=30_000)
    ctx.stream_end()
    ctx.close()
    on, ctx = leased_leg(sv, abi, a.ticks, True, ballast=30_000)
    res.update(leased_tick_us={"inspection_off": us(off), "inspection_on": us(on)}, get_calls_30k=get_calls(ctx))
    ctx.stream_end()
    ctx.close()
    res["rpc_tick_us"] = {"inspection_off": us(rpc_leg(sv, abi, a.ticks, False)), "inspection_on": us(rpc_leg(sv, abi, a.ticks, True))}
    _, ctx = leased_leg(sv, abi, 0, True, ballast=a.big)
    res["get_calls_1m"] = get_calls(ctx, reps=3)
    ctx.stream_end()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
