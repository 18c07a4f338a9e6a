"""Cost of a leased streaming tick against the plain tick of the same build, at the cfg5 shape:
2000 servants, 10k requests, 10k frees by id, 200 heartbeats, 200 reports, 2k renewals per tick,
with about |L| leases in the table (leases far in the future fill it first, in ticks of 10k whose
grants are given back by servant index so that the pool does not fill).
    python tests/tools/lease_tick_cost.py --leases 100000 --ticks 300
prints one JSON line: median wall time per tick (host call to host return) of both modes. Under
`rocprofv3 --kernel-trace --stats -- python tests/tools/lease_tick_cost.py ...` the kernel table
gives the per-kernel split. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

N, HB_REPORTS, RENEWALS = 10_000, 200, 2_000
E64, E32 = np.empty(0, np.uint64), np.empty(0, np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leases", type=int, default=10_000)
    ap.add_argument("--ticks", type=int, default=300)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    rng = np.random.default_rng(5)

    # plain ticks: bench.py's stream (10k requests, 10k releases by servant index, 200 heartbeats)
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, N)
    ctx.stream_begin(es.hb + 8, N, N)
    plain = []
    for t in range(a.ticks + 20):
        who, rows, rel, tk = es.next_tick()
        t0 = time.perf_counter()
        out = ctx.stream_tick(who, rows, rel, tk)
        plain.append(time.perf_counter() - t0)
        es.commit(out)
    ctx.stream_end()
    ctx.close()

    # leased ticks
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, 0)
    max_leases = a.leases + 4 * N
    ctx.stream_begin_leased(es.hb + 8, N, N, max_leases, RENEWALS, N, HB_REPORTS, 1 << 16)
    far = 1 << 40
    held = 0
    while held < a.leases:  # ballast: leases nobody frees; their slots go back by servant index
        who, rows, _, tk = es.next_tick()
        out, ids, _, _, n_l = ctx.stream_tick_leased(who, rows, E32, E64, E64.view(np.int64), E64, E32,
                                                     np.zeros(1, np.uint32), E64, tk, np.full(N, far, np.int64), 0)
        g = out[out < binding.IDX_ENV_NOT_FOUND]
        ctx.stream_tick_leased(E32, rows[:0], g, E64, E64.view(np.int64), E64, E32, np.zeros(1, np.uint32), E64,
                               {k: v[:0] for k, v in tk.items()}, E64.view(np.int64), 0)
        held = n_l
    live_ids, live_srv = E64, E32
    leased = []
    for t in range(a.ticks + 20):
        now = t + 1
        who, rows, _, tk = es.next_tick()
        fr = live_ids
        ren = rng.integers(0, max(held, 1), RENEWALS).astype(np.uint64)  # ballast ids: live, never freed
        rs = ((t * HB_REPORTS + np.arange(HB_REPORTS)) % es.n).astype(np.uint32)
        # every reporting servant lists the grants of the last tick it still holds
        order = np.argsort(live_srv, kind="stable")
        srt = live_srv[order]
        lo, hi = np.searchsorted(srt, rs), np.searchsorted(srt, rs, side="right")
        rid = np.concatenate([live_ids[order[l:h]] for l, h in zip(lo, hi)]) if len(order) else E64
        off = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint32)
        lex = np.full(len(tk["env_id"]), now + 5, np.int64)
        t0 = time.perf_counter()
        out, ids, _, _, n_l = ctx.stream_tick_leased(who, rows, E32, ren, np.full(RENEWALS, far, np.int64), fr, rs,
                                                     off, rid, tk, lex, now)
        leased.append(time.perf_counter() - t0)
        g = out < binding.IDX_ENV_NOT_FOUND
        live_ids, live_srv = ids[g], out[g]
    st = ctx.stats()
    ctx.stream_end()
    ctx.close()
    us = lambda v: round(float(np.median(v[20:])) * 1e6, 1)
    print(json.dumps({"leases": int(n_l), "table_slots": int(1 << int(np.ceil(np.log2(2 * max_leases)))),
                      "ticks": a.ticks, "plain_tick_us": us(plain), "leased_tick_us": us(leased),
                      "last_tick": {k: st[k] for k in ("granted", "leases_freed", "renewals_refused")}}))


if __name__ == "__main__":
    main()
