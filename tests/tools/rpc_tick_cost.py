"""Cost of an rpc tick beside the waiting + leased tick fed the same RPCs expanded by the host, in
one process, at the cfg5 shape: 2000 servants, 4000 RPCs of 2.5 rows on average (about 10k grant
rows) per tick, every grant of the previous tick freed by id, 200 heartbeats, max_waiting 20k.
    python tests/tools/rpc_tick_cost.py --ticks 300
prints one JSON line: median wall time per tick (host call to host return) of
  (a) ydc_stream_tick_waiting_leased with one request row per grant row (the host repeats every RPC's
      personality `rows` times; the time of that expansion is reported apart), and
  (b) ydc_stream_tick_rpc with one row per RPC.
Under `rocprofv3 --kernel-trace --stats -- python tests/tools/rpc_tick_cost.py ...` the kernel table
gives k_rpc_scan, k_rpc_expand, k_rpc_grant and k_rpc_settle beside k_wait_gather and
k_wait_lease_commit. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

RPCS, MAX_ROWS, MAX_WAITING, MAX_LEASES = 4_000, 1 << 16, 20_000, 1 << 18
NIMM, NPRE = np.array([1, 1, 2, 2], np.uint32), np.array([0, 1, 1, 2], np.uint32)  # 2.5 rows on average
E64, E32, Z1 = np.empty(0, np.uint64), np.empty(0, np.uint32), np.zeros(1, np.uint32)
I64 = E64.view(np.int64)


def leg(sv, abi, ticks, rpc):
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, RPCS, 0)
    rng = np.random.default_rng(5)
    if rpc:
        ctx.stream_begin_rpc(es.hb + 8, 16, RPCS, MAX_ROWS, MAX_WAITING, MAX_LEASES, 16, MAX_ROWS, 16, 16)
    else:
        ctx.stream_begin_waiting_leased(es.hb + 8, 16, MAX_ROWS // 2, MAX_WAITING, MAX_LEASES, 16, MAX_ROWS, 16, 16)
    live, cost, expand, granted = E64, [], [], 0
    for t in range(ticks + 20):
        who, rows, _, tk = es.next_tick()
        ni, npf = rng.choice(NIMM, RPCS), rng.choice(NPRE, RPCS)
        tags = np.arange(RPCS, dtype=np.uint64)
        lease_for, dl = np.full(RPCS, 5, np.int64), np.full(RPCS, t, np.int64)  # (nothing waits: both legs alike)
        t0 = time.perf_counter()
        if rpc:
            r = ctx.stream_tick_rpc(who, rows, E32, E64, I64, live, E32, Z1, E64, tk, ni, npf, lease_for, dl, tags, t)
            t1 = t0
            srv = np.concatenate([streaming.rpc_grants(r, 0)[0][:0]] + [r["servants"]])
            g = np.repeat(np.arange(RPCS), ni + npf)
            ok = (np.arange(len(g)) - r["row_off"][g]) < r["n_granted"][g]
            ids, srv = r["task_ids"][ok], srv[ok]
        else:
            k = (ni + npf).astype(np.int64)
            tk2 = {c: np.repeat(v, k) for c, v in tk.items()}
            lf2, dl2, tg2 = np.repeat(lease_for, k), np.repeat(dl, k), np.repeat(tags, k)
            t1 = time.perf_counter()
            r = ctx.stream_tick_waiting_leased(who, rows, E32, E64, I64, live, E32, Z1, E64, tk2, lf2, dl2, tg2, t)
            ok = r[0] < binding.IDX_WAITING
            ids, srv = r[1][ok], r[0][ok]
        t2 = time.perf_counter()
        cost.append(t2 - t1)
        expand.append(t1 - t0)
        live = ids
        es.commit(srv)
        np.subtract.at(es.running, srv, 1)  # (every grant is freed by id in the next tick)
        es.live = es.live[:0]
        granted += len(ids)
    ctx.stream_end()
    ctx.close()
    return cost, expand, granted / (ticks + 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=300)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    us = lambda v: round(float(np.median(v[20:])) * 1e6, 1)
    ca, ea, ga = leg(sv, abi, a.ticks, False)
    cb, _, gb = leg(sv, abi, a.ticks, True)
    print(json.dumps({"ticks": a.ticks, "rpcs_per_tick": RPCS, "grants_per_tick_host_expanded": round(ga),
                      "grants_per_tick_rpc": round(gb), "host_expanded_tick_us": us(ca),
                      "host_expansion_us": us(ea), "rpc_tick_us": us(cb)}))


if __name__ == "__main__":
    main()
